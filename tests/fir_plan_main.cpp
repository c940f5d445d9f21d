// fir_plan_main.cpp -- a stand-alone program over pothoscomms_amd/csrc/fir_plan.hpp for tests/test_fir_plan_cpu.py, which compiles it
// plain and with -fsanitize=address,undefined and runs it as a child process.  It reads one configuration per line from its standard
// input:
//     scalar cplx ctaps ntaps L M taps16 exact
// and prints the planner's result and what each of the four requested algorithms resolves to:
//     K ols_plan auto_min_taps td_algo td_plan parts log2n fold | algo plan refused  (AUTO, DIRECT, OLS_FFT, EXACT)
// The diagnostic overrides keep their defaults.  No device is touched.
#include <cstdio>
#include <initializer_list>

#include "fir_plan.hpp"

int main()
{
    pcx::FirPlanIn c;
    unsigned long long ntaps, L, M;
    int taps16, exact;
    while (std::scanf("%d %d %d %llu %llu %llu %d %d", &c.scalar, &c.cplx, &c.ctaps, &ntaps, &L, &M, &taps16, &exact) == 8) {
        c.ntaps = (size_t)ntaps; c.L = (size_t)L; c.M = (size_t)M;
        c.taps16 = taps16 != 0; c.exact = exact != 0;
        const pcx::FirPlan p = pcx::fir_plan(c);
        std::printf("%zu %d %zu %d %d %d %d %zu |", p.K, p.ols_plan, p.auto_min_taps, p.td_algo, p.td_plan(), p.parts, p.log2n, p.fold);
        for (const int algo : {PCX_FIR_AUTO, PCX_FIR_DIRECT, PCX_FIR_OLS_FFT, PCX_FIR_EXACT}) {
            const pcx::FirChoice ch = pcx::fir_resolve(p, algo);
            std::printf(" %d %d %d", ch.algo, ch.plan, ch.refused ? 1 : 0);
        }
        std::printf("\n");
    }
    return 0;
}
