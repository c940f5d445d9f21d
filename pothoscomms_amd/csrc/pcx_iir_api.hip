// pcx_iir_api.hip -- the pcx_iir handle (include/pcx.h): /comms/iir_filter's taps, its plan and bound, the carried history, and how
// a call is cut for iir.hip.  Every device buffer is allocated at create, sized for order 32 and one slice; a process call allocates
// nothing on the device and walks its outputs in slices, each continuing from the device-resident history left by the one before.
#include <cmath>
#include <vector>

#include "pcx_host.hpp"

using namespace pcx;

namespace {
constexpr size_t kMaxTaps = 66;                       // order 32
constexpr int kMaxNB = 32;
constexpr size_t kImpMax = size_t(1) << 20;           // impulse-response samples the plan may take to decay
const double kDefaultTaps[6] = {0.0676, 0.135, 0.0676, 1, -1.142, 0.412};   // IIRFilter.cpp:57

size_t tab_doubles(int NB) { return 2 * (NB + 1) + 16 * NB + 17 * (size_t)NB * NB; }

using Mat = std::vector<double>;
double inf_norm(const Mat &A, int n)
{
    double m = 0;
    for (int r = 0; r < n; r++) {
        double s = 0;
        for (int c = 0; c < n; c++) s += std::fabs(A[r * n + c]);
        m = std::max(m, s);
    }
    return m;
}

// Schur-Cohn step-down on a[0..N] (a[0] = 1): every reflection coefficient inside the unit circle
bool schur_cohn_stable(const std::vector<double> &a0)
{
    std::vector<double> a = a0;
    for (int m = (int)a.size() - 1; m >= 1; m--) {
        const double k = a[m];
        if (!(std::fabs(k) < 1.0)) return false;
        const double d = 1.0 - k * k;
        std::vector<double> nxt(m);
        for (int i = 0; i < m; i++) nxt[i] = (a[i] - k * a[m - i]) / d;
        a.swap(nxt);
    }
    return true;
}

// l1 norm of the impulse response of num/a (a[0] = 1), run until it has decayed; false when it does not within kImpMax samples
bool impulse_l1(const std::vector<double> &num, const std::vector<double> &a, double *l1, double *peak)
{
    const int N = (int)a.size() - 1;
    std::vector<double> y(kImpMax, 0.0);
    double s = 0, pk = 0;
    for (size_t n = 0; n < kImpMax; n++) {
        double v = n < num.size() ? num[n] : 0.0;
        for (int k = 1; k <= N && (size_t)k <= n; k++) v -= a[k] * y[n - k];
        y[n] = v;
        s += std::fabs(v);
        pk = std::max(pk, std::fabs(v));
        if (!std::isfinite(s)) return false;
        // decayed: the last max(N, 1) samples past the numerator carry less than 2^-60 of the sum
        if (n >= num.size() + (size_t)N && n >= 64) {
            double tail = 0;
            for (int k = 0; k < std::max(N, 1); k++) tail = std::max(tail, std::fabs(y[n - k]));
            if (tail <= s * 0x1p-60) { *l1 = s; *peak = pk; return true; }
        }
    }
    return false;
}
}  // namespace

struct pcx_iir {
    ExecCtx cx;
    IirShape p;
    size_t elem = 0;                  // bytes per stream element
    std::vector<double> taps;         // as given
    double bound = 0;
    DevBuf tab;                       // SCAN tables of the bucket (iir.hip Tab<NB>)
    DevBuf coef;                      // SERIAL: b[0..N], a[0..N], normalised
    DevBuf xh;                        // the last 32 inputs, raw elements, xh[k] = x[-1-k]
    DevBuf ystate;                    // per component the last 32 outputs in double, ystate[c][k] = y[-1-k]
    DevBuf z, tin;                    // per tile of a slice and component: zero-state end state, incoming state (order 32)
    DevBuf ytail;                     // per component the last 32 outputs of a slice
    StageBuf wsIn, wsOut;
};

static int iir_zero_state(pcx_iir *h, hipStream_t st)
{
    PCX_TRY(launch_zero_words(h->xh.p, h->xh.cap / 4, st));
    return launch_zero_words(h->ystate.p, h->ystate.cap / 4, st);
}

// the taps alone, before any handle or device is looked at
static int iir_validate(const double *taps, size_t n)
{
    PCX_CHECK_ARG(n > 0, "IIRFilter::setTaps(): Order cannot 0");
    PCX_CHECK_ARG(taps, "null taps");
    PCX_CHECK_ARG(n % 2 == 0, "IIRFilter::setTaps(): %zu taps: b and a must have the same length", n);
    PCX_CHECK_ARG(n <= kMaxTaps, "IIRFilter::setTaps(): %zu taps: at most %zu (order 32)", n, kMaxTaps);
    for (size_t i = 0; i < n; i++) PCX_CHECK_ARG(std::isfinite(taps[i]), "IIRFilter::setTaps(): tap %zu is not finite", i);
    PCX_CHECK_ARG(taps[n / 2] != 0.0, "IIRFilter::setTaps(): a[0] is 0");
    return PCX_OK;
}

// normalise, choose the plan, build and upload the tables, zero the history: complete on return
static int iir_configure(pcx_iir *h, const double *taps, size_t n)
{
    PCX_TRY(iir_validate(taps, n));
    const int N = (int)(n / 2) - 1;
    const double a0 = taps[N + 1];
    std::vector<double> b(N + 1), a(N + 1);
    for (int k = 0; k <= N; k++) { b[k] = taps[k] / a0; a[k] = taps[N + 1 + k] / a0; }
    a[0] = 1.0;

    int plan = PCX_IIR_SERIAL;
    double S = 0, hA = 0, Hn = 0, hH = 0;
    if (schur_cohn_stable(a) && impulse_l1({1.0}, a, &S, &hA) && impulse_l1(b, a, &Hn, &hH)) plan = PCX_IIR_SCAN;
    int NB = 2;
    while (NB < N) NB *= 2;

    std::vector<double> tab(tab_doubles(kMaxNB), 0.0);
    double bound = 0;
    if (plan == PCX_IIR_SCAN) {
        // companion matrix of the padded order, s = (y[n], ..., y[n-NB+1])
        Mat M((size_t)NB * NB, 0.0);
        for (int k = 0; k < NB; k++) M[k] = k + 1 <= N ? -a[k + 1] : 0.0;
        for (int k = 1; k < NB; k++) M[k * NB + k - 1] = 1.0;
        const size_t oB = 0, oNA = NB + 1, oG = 2 * (NB + 1), oP = oG + 16 * NB, oQ = oP + 9 * (size_t)NB * NB;
        for (int k = 0; k <= NB; k++) { tab[oB + k] = k <= N ? b[k] : 0.0; tab[oNA + k] = k <= N ? -a[k] : 0.0; }
        // M^j for j = 1 ... 4096 by the companion recurrence M^(j+1) = M M^j in long double (squaring a power whose entries are large,
        // as they are for narrow bands, would lose the small powers to cancellation); beyond 4096 by squaring M^4096, which is small
        using LD = long double;
        std::vector<LD> Mj((size_t)NB * NB, 0.0L), nxt((size_t)NB * NB);
        for (size_t e = 0; e < Mj.size(); e++) Mj[e] = M[e];
        double K = 1.0;
        std::vector<LD> P;
        for (int j = 1, d = 0; j <= 4096; j++) {
            if (j <= 16)
                for (int k = 0; k < NB; k++) tab[oG + (j - 1) * NB + k] = (double)Mj[k];
            if (j == (16 << d)) {
                Mat Pd((size_t)NB * NB);
                for (size_t e = 0; e < Pd.size(); e++) Pd[e] = (double)Mj[e];
                std::copy(Pd.begin(), Pd.end(), tab.begin() + oP + (size_t)d * NB * NB);
                K = std::max(K, inf_norm(Pd, NB));
                d++;
            }
            for (int c = 0; c < NB; c++) {
                LD acc = 0;
                for (int k = 0; k < NB; k++) acc += (LD)M[k] * Mj[k * NB + c];
                nxt[c] = acc;
            }
            for (int r = 1; r < NB; r++)
                for (int c = 0; c < NB; c++) nxt[r * NB + c] = Mj[(r - 1) * NB + c];
            if (j == 4096) P = Mj;
            Mj.swap(nxt);
        }
        auto sq = [NB](const std::vector<LD> &A) {
            std::vector<LD> C((size_t)NB * NB, 0.0L);
            for (int r = 0; r < NB; r++)
                for (int k = 0; k < NB; k++)
                    for (int c = 0; c < NB; c++) C[r * NB + c] += A[r * NB + k] * A[k * NB + c];
            return C;
        };
        Mat P8((size_t)NB * NB);
        for (size_t e = 0; e < P8.size(); e++) P8[e] = (double)P[e];
        const double rho = inf_norm(P8, NB);                    // ||M^4096||
        std::vector<LD> Q = P;
        for (int s = 0; s < 6; s++) Q = sq(Q);                  // M^(4096 * 64)
        for (int d = 0; d < 8; d++) {
            Mat Qd((size_t)NB * NB);
            for (size_t e = 0; e < Qd.size(); e++) Qd[e] = (double)Q[e];
            std::copy(Qd.begin(), Qd.end(), tab.begin() + oQ + (size_t)d * NB * NB);
            K = std::max(K, inf_norm(Qd, NB));
            if (d < 7) Q = sq(Q);
        }
        // the a-priori bound per unit of max|x|
        const double u = 0x1p-53;
        double B = 0, Aa = 0;
        for (int k = 0; k <= N; k++) B += std::fabs(b[k]);
        for (int k = 1; k <= N; k++) Aa += std::fabs(a[k]);
        const double Z = S * B;                                // any state or partial response, per unit of max|x|
        const double Kh = std::max(1.0, Aa * hA);             // a state error's largest effect on one output
        double w = 0, r = 1;                                   // the carry walk's errors, decayed by ||M^4096|| per tile
        for (int j = 0; j < 64; j++) { w += r; r = std::min(1.0, r * rho); }
        const double levels = 8 + 1 + 1 + 2 * w + 8;
        bound = u * S * (N + 1) * (2 * B + Aa * Z) + u * levels * (NB + 1) * (K + 1) * Z * Kh;
        if (!std::isfinite(bound)) plan = PCX_IIR_SERIAL;
    }
    std::vector<double> coef(2 * (N + 1));
    for (int k = 0; k <= N; k++) { coef[k] = b[k]; coef[N + 1 + k] = a[k]; }

    PCX_TRY(ctx_quiesce(h->cx));          // an earlier call's kernels may still read the tables and the history
    PCX_TRY(upload(h->tab, tab));
    PCX_TRY(upload(h->coef, coef));
    PCX_TRY(h->xh.ensure_zeroed(h->xh.cap));
    PCX_TRY(h->ystate.ensure_zeroed(h->ystate.cap));
    h->taps.assign(taps, taps + n);
    h->p.N = N;
    h->p.NB = NB;
    h->p.plan = plan;
    h->bound = plan == PCX_IIR_SCAN ? bound : 0.0;
    return PCX_OK;
}

int pcx_iir_create(int scalar, int is_complex, pcx_iir **out)
{
    PCX_CHECK_ARG(out, "null out");
    PCX_CHECK_ARG(valid_scalar(scalar), "IIRFilterFactory: unsupported type (scalar %d)", scalar);
    pcx_iir *h = new (std::nothrow) pcx_iir();
    if (!h) { set_error("out of memory"); return PCX_ERR_STATE; }
    h->p.scalar = scalar;
    h->p.cplx = is_complex != 0;
    h->elem = elem_bytes(scalar, h->p.cplx);
    DeviceScope dev_scope(h->cx.device);
    const size_t tiles = iir_slice() / iir_tile(), hist = (size_t)iir_history();
    int rc = h->tab.ensure(tab_doubles(kMaxNB) * sizeof(double));
    if (rc == PCX_OK) rc = h->coef.ensure(kMaxTaps * sizeof(double));
    if (rc == PCX_OK) rc = h->xh.ensure(hist * 16);
    if (rc == PCX_OK) rc = h->ystate.ensure(2 * hist * sizeof(double));
    if (rc == PCX_OK) rc = h->z.ensure(tiles * 2 * kMaxNB * sizeof(double));
    if (rc == PCX_OK) rc = h->tin.ensure(tiles * 2 * kMaxNB * sizeof(double));
    if (rc == PCX_OK) rc = h->ytail.ensure(2 * hist * sizeof(double));
    if (rc == PCX_OK) rc = iir_configure(h, kDefaultTaps, 6);
    if (rc != PCX_OK) { (void)hipGetLastError(); delete h; return rc; }
    *out = h;
    return PCX_OK;
}
int pcx_iir_destroy(pcx_iir *h) { delete h; return PCX_OK; }

int pcx_iir_set_taps(pcx_iir *h, const double *taps, size_t n)
{
    PCX_TRY(iir_validate(taps, n));
    PCX_CHECK_ARG(h, "null handle");
    DeviceScope dev_scope(h->cx.device);
    return iir_configure(h, taps, n);
}
int pcx_iir_get_taps(const pcx_iir *h, double *taps, size_t cap, size_t *n)
{
    PCX_CHECK_ARG(h && n, "null argument");
    *n = h->taps.size();
    PCX_CHECK_ARG(taps || cap == 0, "null taps");
    for (size_t i = 0; i < std::min(cap, h->taps.size()); i++) taps[i] = h->taps[i];
    return PCX_OK;
}
int pcx_iir_get_plan(const pcx_iir *h, int *plan, double *bound)
{
    PCX_CHECK_ARG(h && plan && bound, "null argument");
    *plan = h->p.plan;
    *bound = h->bound;
    return PCX_OK;
}
int pcx_iir_reset(pcx_iir *h)
{
    PCX_CHECK_ARG(h, "null handle");
    DeviceScope dev_scope(h->cx.device);
    hipStream_t st;
    PCX_TRY(ctx_state_stream(h->cx, &st));
    return iir_zero_state(h, st);
}

int pcx_iir_process_dev(pcx_iir *h, const void *in_dev, void *out_dev, size_t n, void *stream)
{
    PCX_TRACE();
    PCX_CHECK_ARG(h, "null handle");
    if (n == 0) return PCX_OK;
    PCX_CHECK_ARG(in_dev && out_dev, "null buffer");
    // the apply and finish kernels read a slice's inputs after outputs have been written: no byte of the two buffers may be shared
    PCX_CHECK_ARG(buffers_ok(in_dev, n * h->elem, out_dev, n * h->elem, false), "iir_filter: out overlaps in (out == in included)");
    DeviceScope dev_scope(h->cx.device);
    hipStream_t st = as_stream(stream);
    PCX_TRY(ctx_enter(h->cx, st));
    const char *in = static_cast<const char *>(in_dev);
    char *out = static_cast<char *>(out_dev);
    const size_t slice = iir_slice();
    for (size_t off = 0; off < n; off += slice) {
        const size_t m = std::min(slice, n - off);
        PCX_TRY(launch_iir_slice(h->p, in + off * h->elem, out + off * h->elem, m, h->xh.p, static_cast<double *>(h->ystate.p),
                                 static_cast<const double *>(h->tab.p), static_cast<const double *>(h->coef.p),
                                 static_cast<double *>(h->z.p), static_cast<double *>(h->tin.p), static_cast<double *>(h->ytail.p), st));
    }
    return PCX_OK;
}
int pcx_iir_process(pcx_iir *h, const void *in, void *out, size_t n)
{
    PCX_TRACE();
    PCX_CHECK_ARG(h, "null handle");
    if (n == 0) return PCX_OK;
    PCX_CHECK_ARG(in && out, "null buffer");
    const size_t bytes = n * h->elem;
    PCX_CHECK_ARG(buffers_ok(in, bytes, out, bytes, false), "iir_filter: out overlaps in (out == in included)");
    DeviceScope dev_scope(h->cx.device);
    return host_call(h, in, bytes, out, bytes, [&](const void *din, void *dout, hipStream_t st) { return pcx_iir_process_dev(h, din, dout, n, st); });
}
