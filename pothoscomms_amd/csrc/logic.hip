// logic.hip -- the maps that join the pieces of a device-resident chain:
//   /comms/comparator, /comms/const_comparator     math/Comparator.cpp, math/ConstComparator.cpp    out = (a OP b) ? 1 : 0, one byte each
//   /comms/bitwise_unary, /comms/bitwise_binary,
//   /comms/const_bitwise_binary, /comms/bitshift    digital/Bitwise.cpp                              ~ & | ^ << >>
//   /comms/byte_order                               digital/ByteOrder.cpp, ByteOrder.hpp             every scalar reversed
//   /comms/const_arithmetic                         math/ConstArithmetic.cpp                         X+K X-K K-X X*K X/K K/X
// Every result has one right answer and is held to equality: integer results, comparison results and byte permutations by their
// nature, the float and complex operators because they are arith.hip's (arith_ops.hpp), one operand broadcast.
//
// ONE SHAPE.  A buffer is a run of 16-byte UNITS counted from its first byte, at any byte address (unit_io.hpp: gfx950 takes unaligned
// 16-byte accesses at full width, so there is no second kernel for odd addresses -- in a flowgraph a port pointer advances by element
// counts and every element-aligned offset occurs).  A lane owns output unit u: it loads that unit of each of its NIN inputs, applies the
// functor and stores ONE full unit, with the non-temporal hint on both sides (unit_kernel).  The comparators of scalars wider than a
// byte narrow: 16 results come from sizeof(T) input units, which a workgroup loads side by side and exchanges through 4 KiB of LDS
// (compare_kernel).  kBlock x U output units make a chunk; a chunk that lies whole inside the buffer takes the unguarded path, the
// chunk a buffer ends in goes through load_unit / store_unit, which touch single bytes in the last unit only.  An element never
// straddles a unit (element sizes divide 16), so functors see whole elements.
// `out` may be exactly one of the inputs of a same-width map: a lane reads its own units before it writes them and touches no other.
// No scratch, every index 64-bit.
#include "arith_ops.hpp"
#include "pcx_internal.hpp"
#include "unit_io.hpp"

#include <type_traits>

namespace pcx {
namespace {

constexpr int kBlock = 256;

template <int NIN>
struct Ins {
    const unsigned char *p[NIN];
};

template <int NIN, int U, typename F>
__global__ __launch_bounds__(kBlock) void unit_kernel(Ins<NIN> in, unsigned char *out, int64_t n, F f)
{
    const int64_t nunits = (n + 15) / 16;
    constexpr int64_t chunk = (int64_t)kBlock * U;
    const int64_t nchunks = (nunits + chunk - 1) / chunk;
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int64_t base = c * chunk + threadIdx.x;
        if ((c + 1) * chunk * 16 <= n) {          // (the same for every lane of the workgroup)
            uint4 v[U][NIN];
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int i = 0; i < NIN; i++) v[u][i] = nt_load16_any(in.p[i] + 16 * (base + (int64_t)u * kBlock));
#pragma unroll
            for (int u = 0; u < U; u++) nt_store16_any(out + 16 * (base + (int64_t)u * kBlock), f(v[u]));
        } else {
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int64_t unit = base + (int64_t)u * kBlock;
                if (unit >= nunits) break;
                uint4 v[NIN];
#pragma unroll
                for (int i = 0; i < NIN; i++) v[i] = load_unit(in.p[i], 16 * unit, n);
                store_unit(out, 16 * unit, n, f(v));
            }
        }
    }
}

template <int NIN, typename F>
int launch_units(const Ins<NIN> &in, void *out, size_t bytes, F f, hipStream_t st)
{
    constexpr int U = NIN >= 4 ? 1 : 2;         // at least two, at most eight units in flight per lane
    const size_t nunits = (bytes + 15) / 16;
    const unsigned grid = stream_grid(nunits / U + 1, kBlock);
    hipLaunchKernelGGL((unit_kernel<NIN, U, F>), dim3(grid), dim3(kBlock), 0, st, in, static_cast<unsigned char *>(out), (int64_t)bytes, f);
    PCX_LAUNCH_CHECK();
    return PCX_OK;
}

// ---- a unit as 16 / sizeof(T) scalars ----
template <typename T>
struct Lanes {
    static constexpr int N = 16 / (int)sizeof(T);
    T v[N];
    __device__ explicit Lanes(const uint4 &u) { __builtin_memcpy(v, &u, 16); }
    __device__ Lanes() {}
    __device__ uint4 unit() const
    {
        uint4 u;
        __builtin_memcpy(&u, v, 16);
        return u;
    }
};

// ---- bitwise: bit-parallel, on the unit's four words whatever the element type ----
template <int OP>
__device__ __forceinline__ uint32_t bit2(uint32_t a, uint32_t b)
{
    return OP == PCX_BIT_AND ? a & b : OP == PCX_BIT_OR ? a | b : a ^ b;
}
template <int OP>
__device__ __forceinline__ uint4 bit2(const uint4 &a, const uint4 &b)
{
    return make_uint4(bit2<OP>(a.x, b.x), bit2<OP>(a.y, b.y), bit2<OP>(a.z, b.z), bit2<OP>(a.w, b.w));
}
struct BitNot {
    __device__ uint4 operator()(const uint4 (&v)[1]) const { return make_uint4(~v[0].x, ~v[0].y, ~v[0].z, ~v[0].w); }
};
// one pass over NIN inputs: NIN reads and one write of every unit
template <int OP, int NIN>
struct BitFold {
    __device__ uint4 operator()(const uint4 (&v)[NIN]) const
    {
        uint4 acc = v[0];
#pragma unroll
        for (int i = 1; i < NIN; i++) acc = bit2<OP>(acc, v[i]);
        return acc;
    }
};
// the constant repeated over a unit
template <int OP>
struct BitConst {
    uint4 k;
    __device__ uint4 operator()(const uint4 (&v)[1]) const { return bit2<OP>(v[0], k); }
};

// ---- shifts: on the promoted value, narrowed on the store (Bitwise.cpp: out[i] = in[i] << s resp. >> s); the one bitwise operation
// that has to respect element boundaries.  >> of a signed type is arithmetic, as g++'s is ----
template <typename T, bool LEFT>
struct Shift {
    unsigned s;
    __device__ uint4 operator()(const uint4 (&v)[1]) const
    {
        typedef typename std::conditional<(sizeof(T) < 4), int, T>::type P;             // the promoted type
        typedef typename std::make_unsigned<P>::type UP;
        const Lanes<T> a(v[0]);
        Lanes<T> o;
#pragma unroll
        for (int k = 0; k < Lanes<T>::N; k++) {
            const P x = (P)a.v[k];
            o.v[k] = LEFT ? (T)(UP)((UP)x << s) : (T)(x >> s);
        }
        return o.unit();
    }
};

// ---- byte order: every scalar of W bytes reversed ----
template <int W>
struct Swap {
    __device__ static uint32_t rev16(uint32_t w) { return ((w & 0x00ff00ffu) << 8) | ((w >> 8) & 0x00ff00ffu); }
    __device__ uint4 operator()(const uint4 (&v)[1]) const
    {
        const uint4 a = v[0];
        if (W == 2) return make_uint4(rev16(a.x), rev16(a.y), rev16(a.z), rev16(a.w));
        if (W == 4) return make_uint4(__builtin_bswap32(a.x), __builtin_bswap32(a.y), __builtin_bswap32(a.z), __builtin_bswap32(a.w));
        return make_uint4(__builtin_bswap32(a.y), __builtin_bswap32(a.x), __builtin_bswap32(a.w), __builtin_bswap32(a.z));
    }
};

// ---- comparators: C++'s operator on the element type (every ordered comparison and == with a NaN is false, != true) ----
template <typename T, int OP>
__device__ __forceinline__ uint32_t cmp1(T a, T b)
{
    return (OP == PCX_CMP_GT ? a > b : OP == PCX_CMP_LT ? a < b : OP == PCX_CMP_GE ? a >= b : OP == PCX_CMP_LE ? a <= b
            : OP == PCX_CMP_EQ ? a == b : a != b) ? 1u : 0u;
}
// the 1-byte types: a same-width map, unit for unit (and `out` may be the input)
template <typename T, int OP, bool CONST>
struct Compare {
    static constexpr int NIN = CONST ? 1 : 2;
    T k;
    __device__ uint4 operator()(const uint4 (&v)[NIN]) const
    {
        static_assert(sizeof(T) == 1, "wider scalars go through compare_kernel");
        const Lanes<T> a(v[0]);
        const Lanes<T> b(v[NIN - 1]);
        Lanes<unsigned char> o;
#pragma unroll
        for (int j = 0; j < 16; j++) o.v[j] = (unsigned char)cmp1<T, OP>(a.v[j], CONST ? k : b.v[j]);
        return o.unit();
    }
};

// Scalars of R = sizeof(T) >= 2 bytes: 16 results come from R input units.  A workgroup's chunk is 256 output units = 256 R input
// units of each input.  MEASURED (tools/logic_rate.py): a lane that loads the R units of its own output unit puts a
// stride of 16 R bytes between the lanes of every load, and the float64 comparator then ran at 2.3 TB/s against the copy's 5.6.  So
// the loads go side by side instead -- load r of lane t is input unit 256 r + t of the chunk, the whole workgroup on consecutive
// addresses -- the 16 / R result bytes of that unit go to LDS where they belong (byte 16 / R * (256 r + t) of the chunk's 4096 result
// bytes), and behind a barrier lane t picks up output unit t whole: one 16-byte store per lane, as before.  R (2 R with two inputs)
// units are in flight per lane.  `out` never aliases an input here (the host checks).
template <typename T, int OP, bool CONST>
__global__ __launch_bounds__(kBlock) void compare_kernel(const unsigned char *a, const unsigned char *b, unsigned char *out, int64_t n_out, T k)
{
    constexpr int R = (int)sizeof(T), PER = 16 / R;
    typedef typename std::conditional<PER == 2, uint16_t, typename std::conditional<PER == 4, uint32_t, uint64_t>::type>::type Piece;
    __shared__ uint4 stage[kBlock];
    Piece *pieces = reinterpret_cast<Piece *>(stage);
    const int tid = threadIdx.x;
    const int64_t n_in = n_out * R;
    const int64_t nunits = (n_out + 15) / 16;
    const int64_t nchunks = (nunits + kBlock - 1) / kBlock;
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int64_t in0 = 16 * (c * kBlock * R + tid), o0 = 16 * (c * kBlock + tid);
        const bool whole = (c + 1) * kBlock * 16 <= n_out;         // (the same for every lane of the workgroup)
        uint4 va[R], vb[CONST ? 1 : R];
        if (whole) {
#pragma unroll
            for (int r = 0; r < R; r++) {
                va[r] = nt_load16_any(a + in0 + (int64_t)r * kBlock * 16);
                if (!CONST) vb[r] = nt_load16_any(b + in0 + (int64_t)r * kBlock * 16);
            }
        } else {
#pragma unroll
            for (int r = 0; r < R; r++) {
                va[r] = load_unit(a, in0 + (int64_t)r * kBlock * 16, n_in);
                if (!CONST) vb[r] = load_unit(b, in0 + (int64_t)r * kBlock * 16, n_in);
            }
        }
#pragma unroll
        for (int r = 0; r < R; r++) {
            const Lanes<T> x(va[r]);
            Piece p = 0;
            if constexpr (CONST) {
#pragma unroll
                for (int j = 0; j < PER; j++) p |= (Piece)cmp1<T, OP>(x.v[j], k) << (8 * j);
            } else {
                const Lanes<T> y(vb[r]);
#pragma unroll
                for (int j = 0; j < PER; j++) p |= (Piece)cmp1<T, OP>(x.v[j], y.v[j]) << (8 * j);
            }
            pieces[r * kBlock + tid] = p;
        }
        __syncthreads();
        const uint4 o = stage[tid];
        __syncthreads();            // (the next chunk's pieces come behind this chunk's reads)
        if (whole) nt_store16_any(out + o0, o);
        else store_unit(out, o0, n_out, o);
    }
}

// ---- const arithmetic: arith.hip's operators with one operand broadcast; KFIRST: the constant is the left operand (K-X, K/X) ----
template <typename T, int PER, typename Op, bool KFIRST>
struct ArithConst {
    T k[2];
    Op op;
    __device__ uint4 operator()(const uint4 (&v)[1]) const
    {
        const Lanes<T> a(v[0]);
        Lanes<T> o;
#pragma unroll
        for (int e = 0; e < Lanes<T>::N; e += PER) {
            if (KFIRST) op(k, &a.v[e], &o.v[e]);
            else op(&a.v[e], k, &o.v[e]);
        }
        return o.unit();
    }
};

template <typename F>
int launch_same(const void *in, void *out, size_t bytes, F f, hipStream_t st)
{
    Ins<1> ins = {{static_cast<const unsigned char *>(in)}};
    return launch_units<1>(ins, out, bytes, f, st);
}

// ---------------- dispatch ----------------
template <typename T, int OP, bool CONST>
int launch_compare_op(const void *a, const void *b, T k, void *out, size_t n, hipStream_t st)
{
    if constexpr (sizeof(T) == 1) {
        constexpr int NIN = CONST ? 1 : 2;
        Ins<NIN> ins;
        ins.p[0] = static_cast<const unsigned char *>(a);
        ins.p[NIN - 1] = static_cast<const unsigned char *>(CONST ? a : b);
        return launch_units<NIN>(ins, out, n, Compare<T, OP, CONST>{k}, st);
    } else {
        const unsigned grid = stream_grid((n + 15) / 16 + 1, kBlock);
        hipLaunchKernelGGL((compare_kernel<T, OP, CONST>), dim3(grid), dim3(kBlock), 0, st, static_cast<const unsigned char *>(a),
                           static_cast<const unsigned char *>(b), static_cast<unsigned char *>(out), (int64_t)n, k);
        PCX_LAUNCH_CHECK();
        return PCX_OK;
    }
}
template <typename T, bool CONST>
int launch_compare_t(int op, const void *a, const void *b, const void *k, void *out, size_t n, hipStream_t st)
{
    T kv = T();
    if (CONST) std::memcpy(&kv, k, sizeof(T));
    switch (op) {
    case PCX_CMP_GT: return launch_compare_op<T, PCX_CMP_GT, CONST>(a, b, kv, out, n, st);
    case PCX_CMP_LT: return launch_compare_op<T, PCX_CMP_LT, CONST>(a, b, kv, out, n, st);
    case PCX_CMP_GE: return launch_compare_op<T, PCX_CMP_GE, CONST>(a, b, kv, out, n, st);
    case PCX_CMP_LE: return launch_compare_op<T, PCX_CMP_LE, CONST>(a, b, kv, out, n, st);
    case PCX_CMP_EQ: return launch_compare_op<T, PCX_CMP_EQ, CONST>(a, b, kv, out, n, st);
    case PCX_CMP_NE: return launch_compare_op<T, PCX_CMP_NE, CONST>(a, b, kv, out, n, st);
    }
    set_error("comparator: unknown comparison %d", op);
    return PCX_ERR_ARG;
}
template <bool CONST>
int launch_compare_s(int scalar, int op, const void *a, const void *b, const void *k, void *out, size_t n, hipStream_t st)
{
    switch (scalar) {
    case PCX_F64: return launch_compare_t<double, CONST>(op, a, b, k, out, n, st);
    case PCX_F32: return launch_compare_t<float, CONST>(op, a, b, k, out, n, st);
    case PCX_I64: return launch_compare_t<int64_t, CONST>(op, a, b, k, out, n, st);
    case PCX_I32: return launch_compare_t<int32_t, CONST>(op, a, b, k, out, n, st);
    case PCX_I16: return launch_compare_t<int16_t, CONST>(op, a, b, k, out, n, st);
    case PCX_I8: return launch_compare_t<int8_t, CONST>(op, a, b, k, out, n, st);
    case PCX_U64: return launch_compare_t<uint64_t, CONST>(op, a, b, k, out, n, st);
    case PCX_U32: return launch_compare_t<uint32_t, CONST>(op, a, b, k, out, n, st);
    case PCX_U16: return launch_compare_t<uint16_t, CONST>(op, a, b, k, out, n, st);
    case PCX_U8: return launch_compare_t<uint8_t, CONST>(op, a, b, k, out, n, st);
    }
    set_error("comparator: unsupported scalar type %d", scalar);
    return PCX_ERR_ARG;
}

template <int OP, int NIN>
int launch_fold_n(const void *const *ins, void *out, size_t bytes, hipStream_t st)
{
    Ins<NIN> p;
    for (int i = 0; i < NIN; i++) p.p[i] = static_cast<const unsigned char *>(ins[i]);
    return launch_units<NIN>(p, out, bytes, BitFold<OP, NIN>{}, st);
}
template <int OP>
int launch_fold(const void *const *ins, int nin, void *out, size_t bytes, hipStream_t st)
{
    switch (nin) {
    case 2: return launch_fold_n<OP, 2>(ins, out, bytes, st);
    case 3: return launch_fold_n<OP, 3>(ins, out, bytes, st);
    case 4: return launch_fold_n<OP, 4>(ins, out, bytes, st);
    case 5: return launch_fold_n<OP, 5>(ins, out, bytes, st);
    case 6: return launch_fold_n<OP, 6>(ins, out, bytes, st);
    case 7: return launch_fold_n<OP, 7>(ins, out, bytes, st);
    case 8: return launch_fold_n<OP, 8>(ins, out, bytes, st);
    }
    set_error("bitwise: a pass over %d inputs", nin);
    return PCX_ERR_ARG;
}
int launch_fold_op(int op, const void *const *ins, int nin, void *out, size_t bytes, hipStream_t st)
{
    switch (op) {
    case PCX_BIT_AND: return launch_fold<PCX_BIT_AND>(ins, nin, out, bytes, st);
    case PCX_BIT_OR: return launch_fold<PCX_BIT_OR>(ins, nin, out, bytes, st);
    case PCX_BIT_XOR: return launch_fold<PCX_BIT_XOR>(ins, nin, out, bytes, st);
    }
    set_error("bitwise: unknown operation %d over %d inputs", op, nin);
    return PCX_ERR_ARG;
}

template <typename T>
int launch_shift_t(bool left, const void *in, unsigned s, void *out, size_t n, hipStream_t st)
{
    if (left) return launch_same(in, out, n * sizeof(T), Shift<T, true>{s}, st);
    return launch_same(in, out, n * sizeof(T), Shift<T, false>{s}, st);
}

template <typename T, int PER, int OP, bool KFIRST>
int launch_arith_const_op(const void *in, const T *k, void *out, size_t n, hipStream_t st)
{
    typedef typename std::conditional<PER == 2, CplxOp<T, OP>, RealOp<T, OP>>::type Op;
    ArithConst<T, PER, Op, KFIRST> f;
    f.k[0] = k[0];
    f.k[1] = PER == 2 ? k[1] : T();
    return launch_same(in, out, n * PER * sizeof(T), f, st);
}
template <typename T, int PER>
int launch_arith_const_p(int op, const void *in, const void *k, void *out, size_t n, hipStream_t st)
{
    T kv[2] = {T(), T()};
    std::memcpy(kv, k, PER * sizeof(T));
    switch (op) {
    case PCX_ARITHK_X_ADD_K: return launch_arith_const_op<T, PER, PCX_ARITH_ADD, false>(in, kv, out, n, st);
    case PCX_ARITHK_X_SUB_K: return launch_arith_const_op<T, PER, PCX_ARITH_SUB, false>(in, kv, out, n, st);
    case PCX_ARITHK_K_SUB_X: return launch_arith_const_op<T, PER, PCX_ARITH_SUB, true>(in, kv, out, n, st);
    case PCX_ARITHK_X_MUL_K: return launch_arith_const_op<T, PER, PCX_ARITH_MUL, false>(in, kv, out, n, st);
    case PCX_ARITHK_X_DIV_K: return launch_arith_const_op<T, PER, PCX_ARITH_DIV, false>(in, kv, out, n, st);
    case PCX_ARITHK_K_DIV_X: return launch_arith_const_op<T, PER, PCX_ARITH_DIV, true>(in, kv, out, n, st);
    }
    set_error("const arithmetic: unknown operation %d", op);
    return PCX_ERR_ARG;
}
template <typename T>
int launch_arith_const_t(int is_complex, int op, const void *in, const void *k, void *out, size_t n, hipStream_t st)
{
    return is_complex ? launch_arith_const_p<T, 2>(op, in, k, out, n, st) : launch_arith_const_p<T, 1>(op, in, k, out, n, st);
}

}  // namespace

int launch_compare(int scalar, int op, const void *in0, const void *in1, void *out, size_t n, hipStream_t st)
{
    if (n == 0) return PCX_OK;
    return launch_compare_s<false>(scalar, op, in0, in1, nullptr, out, n, st);
}
int launch_compare_const(int scalar, int op, const void *in, const void *k, void *out, size_t n, hipStream_t st)
{
    if (n == 0) return PCX_OK;
    return launch_compare_s<true>(scalar, op, in, nullptr, k, out, n, st);
}

int launch_bitwise(int op, const void *const *ins, size_t nin, void *out, size_t bytes, hipStream_t st)
{
    if (bytes == 0) return PCX_OK;
    if (op == PCX_BIT_NOT) {
        if (nin != 1) {
            set_error("bitwise: NOT takes one input, not %zu", nin);
            return PCX_ERR_ARG;
        }
        return launch_same(ins[0], out, bytes, BitNot{}, st);
    }
    if (nin < 2) {
        set_error("bitwise: operation %d takes two inputs or more, not %zu", op, nin);
        return PCX_ERR_ARG;
    }
    if (nin <= 8) return launch_fold_op(op, ins, (int)nin, out, bytes, st);
    // the first pass takes eight inputs, every further one `out` and up to seven more (the operators are associative and
    // commutative).  An input that IS `out` (the callers admit one) goes into the first pass: a later one would find it overwritten
    std::vector<const void *> order(ins, ins + nin);
    for (size_t i = 1; i < nin; i++)
        if (order[i] == out) { std::swap(order[0], order[i]); break; }
    PCX_TRY(launch_fold_op(op, order.data(), 8, out, bytes, st));
    for (size_t done = 8; done < nin;) {
        const void *group[8] = {out};
        const size_t g = nin - done < 7 ? nin - done : 7;
        for (size_t i = 0; i < g; i++) group[1 + i] = order[done + i];
        PCX_TRY(launch_fold_op(op, group, (int)g + 1, out, bytes, st));
        done += g;
    }
    return PCX_OK;
}

int launch_bitwise_const(int op, int width, const void *in, const void *k, void *out, size_t bytes, hipStream_t st)
{
    if (bytes == 0) return PCX_OK;
    unsigned char rep[16];
    for (int i = 0; i < 16; i += width) std::memcpy(rep + i, k, (size_t)width);
    uint4 kv;
    std::memcpy(&kv, rep, 16);
    switch (op) {
    case PCX_BIT_AND: return launch_same(in, out, bytes, BitConst<PCX_BIT_AND>{kv}, st);
    case PCX_BIT_OR: return launch_same(in, out, bytes, BitConst<PCX_BIT_OR>{kv}, st);
    case PCX_BIT_XOR: return launch_same(in, out, bytes, BitConst<PCX_BIT_XOR>{kv}, st);
    }
    set_error("bitwise: unknown operation %d with a constant", op);
    return PCX_ERR_ARG;
}

int launch_bitshift(int scalar, bool left, const void *in, unsigned shift, void *out, size_t n, hipStream_t st)
{
    if (n == 0) return PCX_OK;
    switch (scalar) {
    case PCX_I64: return launch_shift_t<int64_t>(left, in, shift, out, n, st);
    case PCX_I32: return launch_shift_t<int32_t>(left, in, shift, out, n, st);
    case PCX_I16: return launch_shift_t<int16_t>(left, in, shift, out, n, st);
    case PCX_I8: return launch_shift_t<int8_t>(left, in, shift, out, n, st);
    case PCX_U64: return launch_shift_t<uint64_t>(left, in, shift, out, n, st);
    case PCX_U32: return launch_shift_t<uint32_t>(left, in, shift, out, n, st);
    case PCX_U16: return launch_shift_t<uint16_t>(left, in, shift, out, n, st);
    case PCX_U8: return launch_shift_t<uint8_t>(left, in, shift, out, n, st);
    }
    set_error("bitshift: unsupported scalar type %d", scalar);
    return PCX_ERR_ARG;
}

int launch_byteswap(int width, const void *in, void *out, size_t n_scalars, hipStream_t st)
{
    if (n_scalars == 0) return PCX_OK;
    switch (width) {
    case 2: return launch_same(in, out, n_scalars * 2, Swap<2>{}, st);
    case 4: return launch_same(in, out, n_scalars * 4, Swap<4>{}, st);
    case 8: return launch_same(in, out, n_scalars * 8, Swap<8>{}, st);
    }
    set_error("byte order: unsupported scalar width %d", width);
    return PCX_ERR_ARG;
}

int launch_arith_const(int scalar, int is_complex, int op, const void *in, const void *k, void *out, size_t n, hipStream_t st)
{
    if (n == 0) return PCX_OK;
    switch (scalar) {
    case PCX_F64: return launch_arith_const_t<double>(is_complex, op, in, k, out, n, st);
    case PCX_F32: return launch_arith_const_t<float>(is_complex, op, in, k, out, n, st);
    case PCX_I64: return launch_arith_const_t<int64_t>(is_complex, op, in, k, out, n, st);
    case PCX_I32: return launch_arith_const_t<int32_t>(is_complex, op, in, k, out, n, st);
    case PCX_I16: return launch_arith_const_t<int16_t>(is_complex, op, in, k, out, n, st);
    case PCX_I8: return launch_arith_const_t<int8_t>(is_complex, op, in, k, out, n, st);
    case PCX_U64: return launch_arith_const_t<uint64_t>(is_complex, op, in, k, out, n, st);
    case PCX_U32: return launch_arith_const_t<uint32_t>(is_complex, op, in, k, out, n, st);
    case PCX_U16: return launch_arith_const_t<uint16_t>(is_complex, op, in, k, out, n, st);
    case PCX_U8: return launch_arith_const_t<uint8_t>(is_complex, op, in, k, out, n, st);
    }
    set_error("const arithmetic: unsupported scalar type %d", scalar);
    return PCX_ERR_ARG;
}

}  // namespace pcx
