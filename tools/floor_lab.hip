// floor_lab.hip -- memory and issue FLOORS of the overlap-save variants that sit furthest below the HBM roof:
// the fused chain (fmchain), the decimating FIR (decim8) and the interpolating FIR (interp4).  Diagnostic, not part of the product.
//
// For each of them the harness runs a kernel that has the product kernel's SHAPE and none of its mathematics:
//   * the same launch (256 lanes, the same workgroups per CU, the same persistent grid and block walk),
//   * the same loads (sixteen -- or four -- 2 KiB rows per block through a buffer descriptor, the interior rows non-temporal) and
//     the same stores (rows of the block's valid outputs, streaming policy),
//   * the same LDS footprint (so that no more workgroups fit than the product kernel gets),
// in three rows per kernel:
//   mem    loads and stores alone: what the memory system gives this access pattern at this occupancy;
//   dose   the same, with the product kernel's VALU instruction count per wave and block (PMC, profiles/) spent between the loads
//          and the stores as INDEPENDENT packed FMAs -- no exchange, no barrier, no dependency: the issue floor on top of memory;
//   dose+x the same, with the kernel's LDS exchanges (barrier + 16 ds_write_b64 + 16 ds_read_b64 per exchange) between the doses.
// The product kernels themselves -- on the bench's data and on all-zero input (same instructions, no switching energy) -- are timed
// next to these rows by tools/floor_table.py through the product library, on the same box in the same call.
//
// Build: make -C tools floor_lab        Run: tools/floor_lab [seconds-per-row]
//                                        tools/floor_lab <seconds-per-row> wide [rounds]: the headline's shape, 8- against 16-byte rows (below)
//                                        tools/floor_lab <seconds-per-row> rows [rounds] [e3|e4|e5]: the headline's shape, 8-byte rows, which rows
//                                            are loaded and stored on the default cache policy (below); the last argument names the load mask of the store sweep
//                                        tools/floor_lab 0 rows pmc: twenty launches each of the n1 / n2 / n4 / n8 `mem` rows and nothing else, for a counter run
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../pothoscomms_amd/csrc/pcx_sched.hpp"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

typedef float cf __attribute__((ext_vector_type(2)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void *p, unsigned bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, (int)bytes, 0x00020000);
}

struct Shape {
    const char *name;
    int occ;              // workgroups per CU of the product kernel
    unsigned grid;        // its persistent grid
    int rows_in;          // 2 KiB rows loaded per block (16: a 4096-sample window; 4: the interpolator's 1024-sample window)
    size_t in_step;       // input samples a block advances by
    int out_elem_bytes;   // 8 (complex_float32) or 4 (float32)
    size_t out_per_block; // output elements per block
    int group;            // blocks per pass of the walk (the batched kernels take G blocks, then store them together)
    int valu;             // VALU instructions per wave and block of the product kernel (SQ_INSTS_VALU / waves / blocks, profiles/)
    int exchanges;        // LDS exchanges (barrier + full image write + read) per block
    size_t nblocks;
    double alg_bytes;     // algorithmic bytes per launch
};

// DOSE: N independent packed FMAs per lane on the sixteen loaded values (each is one wave-level VALU instruction)
__device__ __forceinline__ void dose(cf (&v)[16], int n, cf c)
{
    for (int i = 0; i < n; i += 16) {
#pragma unroll
        for (int q = 0; q < 16; q++) asm volatile("v_pk_fma_f32 %0, %0, %1, %1" : "+v"(v[q]) : "v"(c));
    }
}

template <int OCC, int ROWS, int MODE>     // MODE 0 mem, 1 dose, 2 dose + exchanges
__global__ __launch_bounds__(256, OCC) void floor_kernel(const cf *__restrict__ in, size_t in_elems, unsigned char *__restrict__ out, Shape s, float k)
{
    __shared__ cf lds[4608 + 64];        // the product kernels' image: 36,864 bytes (+ the chain's edge slots)
    const int j = threadIdx.x;
    const cf c = {k, k};
    const size_t ngroups = (s.nblocks + s.group - 1) / s.group;
    for (size_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        cf acc[16];
#pragma unroll
        for (int q = 0; q < 16; q++) acc[q] = cf{0.f, 0.f};
        for (int g = 0; g < s.group; g++) {
            const size_t b = grp * s.group + g;
            if (b >= s.nblocks) break;
            cf v[16];
#pragma unroll
            for (int q = 0; q < 16; q++) v[q] = cf{0.f, 0.f};
            const size_t first = b * s.in_step;
            const size_t left = in_elems - first;
            const size_t want = (size_t)ROWS * 256;
            const __amdgpu_buffer_rsrc_t rs = make_rsrc(in + first, (unsigned)((left < want ? left : want) * 8));
#pragma unroll
            for (int r = 0; r < ROWS; r++) {
                const u32x2 t = (r == 0 || r == ROWS - 1) ? __builtin_amdgcn_raw_buffer_load_b64(rs, j * 8, 2048 * r, 0)
                                                          : __builtin_amdgcn_raw_buffer_load_b64(rs, j * 8, 2048 * r, 2);
                v[r] = cf{__uint_as_float(t.x), __uint_as_float(t.y)};
            }
            if (MODE >= 1) {
                const int per = s.valu / (MODE == 2 ? s.exchanges + 1 : 1);
                dose(v, per, c);
                if (MODE == 2) {
                    for (int x = 0; x < s.exchanges; x++) {
#pragma unroll
                        for (int q = 0; q < 16; q++) lds[17 * j + q] = v[q];
                        __syncthreads();
#pragma unroll
                        for (int q = 0; q < 16; q++) v[q] = lds[j + (j >> 4) + 272 * q];
                        dose(v, per, c);
                        __syncthreads();
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < 16; q++) acc[q] = acc[q] + v[q];
        }
        // the group's outputs are contiguous in the output stream: rows of 256 elements, one element per lane and row
        const size_t o0 = grp * s.group * s.out_per_block;
        const size_t total = (grp * s.group + s.group <= s.nblocks ? (size_t)s.group : s.nblocks - grp * s.group) * s.out_per_block;
        const __amdgpu_buffer_rsrc_t ws = make_rsrc(out + o0 * s.out_elem_bytes, (unsigned)(total * s.out_elem_bytes));
        const int nrows = (int)((total + 255) / 256);
        for (int r = 0; r < nrows; r++) {
            const cf y = acc[r & 15];
            if (s.out_elem_bytes == 8) __builtin_amdgcn_raw_buffer_store_b64(u32x2{__float_as_uint(y.x), __float_as_uint(y.y)}, ws, j * 8, 2048 * r, 2);
            else __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(y.x), ws, j * 4, 1024 * r, 2);
        }
    }
}

// ---- the headline's launch shape with 16-byte stream rows (profiles/r07/floor_wide_rows.txt) -----------------------------------
// fir255 as the product runs it: 1024 workgroups, blocks DEALT (pcx_sched.hpp), S = 3840, the block's first 2 KiB row dropped by the
// store descriptor's range check.  WIDE = false: sixteen 8-byte rows per lane, lane j on column j (the product's accesses).
// WIDE = true: eight 16-byte accesses per lane, access k = rows 2k (lanes 0-31 of a wave) and 2k+1 (lanes 32-63) at columns
// 64w + 2(l & 31) and the next; with SWAP the half-wave exchange that leaves every lane with both rows of ONE column
// (v_permlane32_swap: vdst = the lane's first element, src = its second) is spent on the way in and on the way out, 32 per block.
// LROWS: bit r set = row r of the window is loaded on the default cache policy, clear = non-temporal (a 16-byte access takes the default
// policy when either of its two rows has its bit).  ends(n) = n rows at either end: ends(1) = the product until round 7 (only rows 0 and
// 15 are shared with a neighbouring block), ends(2) = the product since, ends(8) = every row.  SROWS: the same for the rows stored
// (row 0 is never stored: its bit means nothing); 0 = every store non-temporal, as the product stores.
constexpr unsigned ends(int n) { return ((1u << n) - 1u) | (((1u << n) - 1u) << (16 - n)); }
__device__ __forceinline__ void half_swap(cf &first, cf &second)
{
    unsigned a[2] = {__float_as_uint(first.x), __float_as_uint(first.y)}, b[2] = {__float_as_uint(second.x), __float_as_uint(second.y)};
#pragma unroll
    for (int d = 0; d < 2; d++) {
        const auto r = __builtin_amdgcn_permlane32_swap(a[d], b[d], false, false);
        a[d] = r[0]; b[d] = r[1];
    }
    first = cf{__uint_as_float(a[0]), __uint_as_float(a[1])};
    second = cf{__uint_as_float(b[0]), __uint_as_float(b[1])};
}

template <bool WIDE, unsigned LROWS, unsigned SROWS, int MODE, bool SWAP>     // MODE 0 mem, 1 dose
__global__ __launch_bounds__(256, 4) void dealt_kernel(const cf *__restrict__ in, size_t in_elems, unsigned char *__restrict__ out, Shape s, float k,
                                                      pcx::SchedState *__restrict__ sched)
{
    __shared__ cf lds[4608 + 64];
    __shared__ unsigned sched_slot;
    const int j = threadIdx.x, l = j & 63;
    const cf c = {k, k};
    if (j == 0) lds[0] = c;              // (the image is part of the shape: keep it allocated)
    pcx::BlockDealer deal;
    if (!deal.begin(sched, &sched_slot, s.nblocks, j)) { deal.finish(j); return; }
    const int col = WIDE ? (j & ~63) + 2 * (l & 31) : j;
    const int lane_off = WIDE ? col * 8 + (l >> 5) * 2048 : j * 8;
    for (;;) {
        const size_t b = deal.block();
        cf v[16];
        const size_t first = b * s.in_step;
        const size_t left = in_elems - first;
        const __amdgpu_buffer_rsrc_t rs = make_rsrc(in + first, (unsigned)((left < 4096 ? left : 4096) * 8));
        if (WIDE) {
#pragma unroll
            for (int p = 0; p < 8; p++) {
                const u32x4 t = ((LROWS >> (2 * p)) & 3u) ? __builtin_amdgcn_raw_buffer_load_b128(rs, lane_off, 4096 * p, 0)
                                                   : __builtin_amdgcn_raw_buffer_load_b128(rs, lane_off, 4096 * p, 2);
                v[2 * p] = cf{__uint_as_float(t.x), __uint_as_float(t.y)};
                v[2 * p + 1] = cf{__uint_as_float(t.z), __uint_as_float(t.w)};
            }
            if (SWAP) {
#pragma unroll
                for (int p = 0; p < 8; p++) half_swap(v[2 * p], v[2 * p + 1]);
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const bool plain = (LROWS >> r) & 1u;
                const u32x2 t = plain ? __builtin_amdgcn_raw_buffer_load_b64(rs, lane_off, 2048 * r, 0)
                                      : __builtin_amdgcn_raw_buffer_load_b64(rs, lane_off, 2048 * r, 2);
                v[r] = cf{__uint_as_float(t.x), __uint_as_float(t.y)};
            }
        }
        asm volatile("" : : "v"(v[0]));      // row 0 is loaded as the product loads it, though none of it is stored
        if (MODE >= 1) dose(v, 16, c);
        deal.draw(j);
        if (MODE >= 1) dose(v, s.valu - 16, c);
        deal.publish(j);
        __syncthreads();
        // rows 1 .. 15 of the block are outputs b S .. b S + 3839; row 0 lies in front of the descriptor: its offsets wrap and are dropped
        const size_t o0 = b * s.out_per_block;
        const size_t room = s.nblocks * s.out_per_block - o0;      // (the lab's last block is a full one)
        const __amdgpu_buffer_rsrc_t ws = make_rsrc(out + o0 * 8, (unsigned)((room < s.out_per_block ? room : s.out_per_block) * 8));
        if (WIDE) {
            if (SWAP) {
#pragma unroll
                for (int p = 0; p < 8; p++) half_swap(v[2 * p], v[2 * p + 1]);
            }
            const unsigned vbase = (unsigned)(lane_off - 2048);
#pragma unroll
            for (int p = 0; p < 8; p++) {
                const u32x4 y = {__float_as_uint(v[2 * p].x), __float_as_uint(v[2 * p].y), __float_as_uint(v[2 * p + 1].x), __float_as_uint(v[2 * p + 1].y)};
                if ((SROWS >> (2 * p)) & 3u) __builtin_amdgcn_raw_buffer_store_b128(y, ws, (int)(vbase + 4096u * p), 0, 0);      // (folds per row once unrolled: no branch)
                else __builtin_amdgcn_raw_buffer_store_b128(y, ws, (int)(vbase + 4096u * p), 0, 2);
            }
        } else {
            const unsigned vbase = (unsigned)(lane_off - 2048);
#pragma unroll
            for (int r = 1; r < 16; r++) {
                const u32x2 y = {__float_as_uint(v[r].x), __float_as_uint(v[r].y)};
                if ((SROWS >> r) & 1u) __builtin_amdgcn_raw_buffer_store_b64(y, ws, (int)(vbase + 2048u * r), 0, 0);
                else __builtin_amdgcn_raw_buffer_store_b64(y, ws, (int)(vbase + 2048u * r), 0, 2);
            }
        }
        if (!deal.advance()) break;
        __syncthreads();                 // the slot is rewritten by the next block's publish
    }
    deal.finish(j);
}

template <bool WIDE, unsigned LROWS, unsigned SROWS, int MODE, bool SWAP>
static double run_dealt(const Shape &s, const cf *in, size_t in_elems, unsigned char *out, double seconds, float k, pcx::SchedState *sched)
{
    auto launch = [&]() { hipLaunchKernelGGL((dealt_kernel<WIDE, LROWS, SROWS, MODE, SWAP>), dim3(s.grid), dim3(256), 0, 0, in, in_elems, out, s, k, sched); };
    if (seconds <= 0) {      // a counter run: twenty launches, no timing
        for (int i = 0; i < 20; i++) launch();
        CK(hipDeviceSynchronize());
        return 0;
    }
    for (int i = 0; i < 200; i++) launch();
    CK(hipDeviceSynchronize());
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    int n = 0;
    const auto t0 = std::chrono::steady_clock::now();
    CK(hipEventRecord(e0, 0));
    do {
        for (int i = 0; i < 100; i++) launch();
        n += 100;
        CK(hipStreamSynchronize(0));
    } while (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < seconds);
    CK(hipEventRecord(e1, 0));
    CK(hipEventSynchronize(e1));
    float ms = 0;
    CK(hipEventElapsedTime(&ms, e0, e1));
    CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
    return ms / n;
}

template <int OCC, int ROWS>
static double run(const Shape &s, int mode, const cf *in, size_t in_elems, unsigned char *out, double seconds, float k)
{
    auto launch = [&]() {
        if (mode == 0) hipLaunchKernelGGL((floor_kernel<OCC, ROWS, 0>), dim3(s.grid), dim3(256), 0, 0, in, in_elems, out, s, k);
        else if (mode == 1) hipLaunchKernelGGL((floor_kernel<OCC, ROWS, 1>), dim3(s.grid), dim3(256), 0, 0, in, in_elems, out, s, k);
        else hipLaunchKernelGGL((floor_kernel<OCC, ROWS, 2>), dim3(s.grid), dim3(256), 0, 0, in, in_elems, out, s, k);
    };
    for (int i = 0; i < 200; i++) launch();
    CK(hipDeviceSynchronize());
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    int n = 0;
    const auto t0 = std::chrono::steady_clock::now();
    CK(hipEventRecord(e0, 0));
    do {
        for (int i = 0; i < 100; i++) launch();
        n += 100;
        CK(hipStreamSynchronize(0));
    } while (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < seconds);
    CK(hipEventRecord(e1, 0));
    CK(hipEventSynchronize(e1));
    float ms = 0;
    CK(hipEventElapsedTime(&ms, e0, e1));
    return ms / n;
}

int main(int argc, char **argv)
{
    const double seconds = argc > 1 ? atof(argv[1]) : 1.0;
    const size_t C = 64u << 20;
    cf *in;
    unsigned char *out;
    CK(hipMalloc(&in, (C + 8192) * 8));
    CK(hipMalloc(&out, (C + 8192) * 8));
    {   // real data in the input: the loads' switching energy is part of the floor
        std::vector<float> h((C + 8192) * 2);
        unsigned long long z = 88172645463325252ull;
        for (auto &x : h) { z ^= z << 13; z ^= z >> 7; z ^= z << 17; x = (float)((int)(z >> 40) - (1 << 23)) * (1.0f / (1 << 23)); }
        CK(hipMemcpy(in, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    }
    // shapes: block geometry from the launchers (fir_ols.hip, fir_ols_decim.hip), VALU per wave and block from profiles/r03/*_rocprofv3_summary.txt
    const Shape fm{"fmchain (127 taps, 64 Mi)", 4, 1024, 16, 3968, 4, 3968, 1, 952, 3, (C + 3967) / 3968, 12.0 * C};
    const Shape dc{"decim8 (255 taps, 64 Mi in)", 3, 729, 16, 3840, 8, 480, 4, 402, 3, (C + 3839) / 3840, 9.0 * C};
    const Shape ip{"interp4 (255 taps/phase, 16 Mi in)", 3, 729, 4, 768, 8, 3072, 4, 447, 3, (C / 4 + 767) / 768, 8.0 * (C / 4) + 8.0 * C};
    const Shape fr{"fir255 (255 taps, 64 Mi) for scale", 4, 1024, 16, 3840, 8, 3840, 1, 661, 3, (C + 3839) / 3840, 16.0 * C};
    printf("%-38s %-10s %10s %8s %8s\n", "shape", "row", "ms/launch", "GB/s", "of 8 TB/s");
    auto row = [&](const Shape &s, const char *what, double ms) {
        if (ms <= 0) { printf("%-38s %-10s (launched, not timed)\n", s.name, what); return; }
        printf("%-38s %-10s %10.4f %8.0f %8.4f\n", s.name, what, ms, s.alg_bytes / ms / 1e6, s.alg_bytes / ms / 1e6 / 8000.0);
        fflush(stdout);
    };
    const char *names[3] = {"mem", "dose", "dose+x"};
    if (argc > 2 && std::string(argv[2]) == "sweep") {
        // what an LDS exchange costs the decimator's shape, and what a fourth workgroup per CU would buy: exchanges per block 0..3 at
        // three and at four workgroups per CU (the product kernel: three exchanges' worth at three per CU, 170 VGPRs)
        for (int occ = 3; occ <= 4; occ++)
            for (int x = 0; x <= 3; x++) {
                Shape t = dc;
                t.occ = occ; t.grid = occ == 3 ? 729 : 1024; t.exchanges = x;
                char what[32];
                snprintf(what, sizeof what, "occ%d x%d", occ, x);
                const double ms = x == 0 ? (occ == 3 ? run<3, 16>(t, 1, in, C + 4096, out, seconds, 1e-3f) : run<4, 16>(t, 1, in, C + 4096, out, seconds, 1e-3f))
                                         : (occ == 3 ? run<3, 16>(t, 2, in, C + 4096, out, seconds, 1e-3f) : run<4, 16>(t, 2, in, C + 4096, out, seconds, 1e-3f));
                row(t, what, ms);
            }
        for (int occ = 3; occ <= 4; occ++)
            for (int x = 0; x <= 3; x++) {
                Shape t = ip;
                t.occ = occ; t.grid = occ == 3 ? 729 : 1024; t.exchanges = x;
                char what[32];
                snprintf(what, sizeof what, "occ%d x%d", occ, x);
                const double ms = x == 0 ? (occ == 3 ? run<3, 4>(t, 1, in, C / 4 + 4096, out, seconds, 1e-3f) : run<4, 4>(t, 1, in, C / 4 + 4096, out, seconds, 1e-3f))
                                         : (occ == 3 ? run<3, 4>(t, 2, in, C / 4 + 4096, out, seconds, 1e-3f) : run<4, 4>(t, 2, in, C / 4 + 4096, out, seconds, 1e-3f));
                row(t, what, ms);
            }
        return 0;
    }
    if (argc > 2 && std::string(argv[2]) == "wide") {
        // tools/floor_lab <seconds> wide [rounds]: the headline's shape, 8-byte rows against 16-byte rows, the rows interleaved round by round
        const int rounds = argc > 3 ? atoi(argv[3]) : 4;
        pcx::SchedState *sched;
        CK(hipMalloc(&sched, 4096));
        CK(hipMemset(sched, 0, 4096));
        Shape t = fr;
        t.nblocks = C / 3840;            // full blocks only: every window inside the buffer, every output row whole
        t.alg_bytes = 16.0 * 3840 * t.nblocks;
        t.name = "fir255 dealt";
        for (int r = 0; r < rounds; r++) {
            row(t, "mem", run<4, 16>(t, 0, in, C + 4096, out, seconds, 1e-3f));           // the grid-stride row of the table above
#define DEALT_ROW(NAME, WIDE, NOV, MODE, SWAP) row(t, NAME, run_dealt<WIDE, ends(NOV), 0u, MODE, SWAP>(t, in, C + 4096, out, seconds, 1e-3f, sched))
            DEALT_ROW("mem8 n1", false, 1, 0, false);            // the product's accesses
            DEALT_ROW("mem8 n2", false, 2, 0, false);
            DEALT_ROW("mem16 n2", true, 2, 0, false);            // 16-byte rows, the same policy per row pair
            DEALT_ROW("mem16s n2", true, 2, 0, true);
            DEALT_ROW("mem8 n4", false, 4, 0, false);
            DEALT_ROW("mem16 n4", true, 4, 0, false);
            DEALT_ROW("mem8 n8", false, 8, 0, false);
            DEALT_ROW("mem16 n8", true, 8, 0, false);
            DEALT_ROW("dose8 n1", false, 1, 1, false);
            DEALT_ROW("dose8 n2", false, 2, 1, false);
            DEALT_ROW("dose16s n2", true, 2, 1, true);
            DEALT_ROW("dose8 n4", false, 4, 1, false);
#undef DEALT_ROW
        }
        return 0;
    }
    if (argc > 2 && std::string(argv[2]) == "rows") {
        // tools/floor_lab <seconds> rows [rounds] [e3|e4|e5]: the headline's shape, 8-byte rows, by WHICH rows take the default cache policy;
        // the rows interleaved round by round (profiles/r08/floor_row_policy.txt)
        const bool pmc = argc > 3 && std::string(argv[3]) == "pmc";
        const int rounds = pmc ? 1 : argc > 3 ? atoi(argv[3]) : 4;
        const std::string sbase = argc > 4 ? argv[4] : "e4";
        pcx::SchedState *sched;
        CK(hipMalloc(&sched, 4096));
        CK(hipMemset(sched, 0, 4096));
        Shape t = fr;
        t.nblocks = C / 3840;            // full blocks only: every window inside the buffer, every output row whole
        t.alg_bytes = 16.0 * 3840 * t.nblocks;
        t.name = "fir255 dealt";
#define ROWS_ROW(NAME, LROWS, SROWS, MODE) row(t, NAME, run_dealt<false, LROWS, SROWS, MODE, false>(t, in, C + 4096, out, pmc ? 0.0 : seconds, 1e-3f, sched))
#define ROWS_BOTH(NAME, LROWS, SROWS) do { ROWS_ROW("mem8 " NAME, LROWS, SROWS, 0); if (!pmc) ROWS_ROW("dose8 " NAME, LROWS, SROWS, 1); } while (0)
        for (int r = 0; r < rounds; r++) {
            // n default-policy rows at either end
            ROWS_BOTH("n1", ends(1), 0u);
            ROWS_BOTH("n2", ends(2), 0u);            // the product
            ROWS_BOTH("n4", ends(4), 0u);
            ROWS_BOTH("n8", ends(8), 0u);
            if (pmc) break;
            ROWS_BOTH("n3", ends(3), 0u);
            ROWS_BOTH("n5", ends(5), 0u);
            ROWS_BOTH("n6", ends(6), 0u);
            // the same COUNT elsewhere: eight rows as 4 + 4 (n4 above), as every other row (0 2 4 6 9 11 13 15), as 2 + 6 and as 6 + 2;
            // four rows as 2 + 2 (n2 above) and as 1 + 2 in the middle + 1; eight rows as 1 + 6 in the middle + 1
            ROWS_BOTH("alt8", 0xAA55u, 0u);
            ROWS_BOTH("2+6", 0xFC03u, 0u);
            ROWS_BOTH("6+2", 0xC03Fu, 0u);
            ROWS_BOTH("1+mid2+1", 0x8181u, 0u);
            ROWS_BOTH("1+mid6+1", 0x87E1u, 0u);
            // stored rows on the default policy, with the load mask named on the command line: the four / eight at the ends of the
            // fifteen stored rows (1 2 14 15 / 1-4 12-15), and all fifteen
#define STORE_SWEEP(TAG, LROWS) do { ROWS_BOTH(TAG " st4", LROWS, 0xC006u); ROWS_BOTH(TAG " st8", LROWS, 0xF01Eu); ROWS_BOTH(TAG " st15", LROWS, 0xFFFEu); } while (0)
            if (sbase == "e3") STORE_SWEEP("n3", ends(3));
            else if (sbase == "e5") STORE_SWEEP("n5", ends(5));
            else STORE_SWEEP("n4", ends(4));
#undef STORE_SWEEP
        }
#undef ROWS_BOTH
#undef ROWS_ROW
        return 0;
    }
    for (int m = 0; m < 3; m++) row(fr, names[m], run<4, 16>(fr, m, in, C + 4096, out, seconds, 1e-3f));
    for (int m = 0; m < 3; m++) row(fm, names[m], run<4, 16>(fm, m, in, C + 4096, out, seconds, 1e-3f));
    for (int m = 0; m < 3; m++) row(dc, names[m], run<3, 16>(dc, m, in, C + 4096, out, seconds, 1e-3f));
    for (int m = 0; m < 3; m++) row(ip, names[m], run<3, 4>(ip, m, in, C / 4 + 4096, out, seconds, 1e-3f));
    return 0;
}
