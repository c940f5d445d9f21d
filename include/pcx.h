/*
 * pcx.h -- C ABI of libpcx_hip.so: the MI355X (gfx950) device path behind the
 * PothosComms streaming-DSP blocks.
 *
 * The reference has no FFI: each block is a C++ class whose work() runs the
 * arithmetic inline.  This header is the boundary a Pothos
 * plugin TU (pothos_plugin/) calls from inside
 * work()/setters instead of those loops.  One entry point per reference
 * loop / setter it replaces, cited as <file>:<line> of the reference tree.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ types, no exceptions; every call
 *     returns PCX_OK (0) or a negative pcx_status and records a message
 *     retrievable with pcx_last_error() (thread-local).
 *   - scalar types are pcx_scalar codes; a complex stream is interleaved
 *     (re, im) pairs of that scalar -- the memory layout of std::complex<T>.
 *   - "elements" are stream elements (one complex pair = one element).
 *   - *_dev variants take DEVICE pointers and a hipStream_t (as void*) and
 *     only enqueue work; the plain variants take HOST pointers (the
 *     BufferChunk memory of a Pothos port) and return after the result is in
 *     `out`.  Page-locked host memory (pcx_host_alloc, hipHostMalloc,
 *     hipHostRegister -- what the module's BufferManagers hand out) is
 *     processed IN PLACE: the kernels read and write it over PCIe, both
 *     directions at once, on a launch shape of their own (a link-bound call
 *     runs on a few dozen workgroups that walk many pieces each, so that one
 *     piece's loads travel beside the previous piece's stores).  Memory the
 *     FRAMEWORK owns can be page-locked where it lies (pcx_host_register,
 *     pcx_host_register_mapping).  Pageable memory is staged through a
 *     page-locked bounce buffer and a device workspace owned by the handle
 *     (CPU copy, pinned H2D, kernel, pinned D2H, CPU copy).
 *   - *_create and the setters return with everything they zero or upload
 *     COMPLETE on the device: a handle can be used at once on any stream.
 *   - every handle owns a non-blocking stream for its host-pointer calls, so
 *     blocks on different actor threads overlap on the device; nothing runs
 *     on the legacy default stream.
 *   - handles are not thread-safe; one handle per block instance, exactly as
 *     Pothos serialises work() and setters on one actor.
 *   - a handle is bound to ONE device: the device current (pcx_set_device) on
 *     the thread that CREATES it.  Later calls from any thread run on that
 *     device and leave the caller's current device unchanged, so a single
 *     Pothos process can place blocks on different GPUs.  The stateless maps
 *     run on the calling thread's current device.
 *   - ordering: a *_dev call on another stream than the handle's previous
 *     call is ordered behind it (an event), carried state and all; setters
 *     that rewrite device tables first wait for the handle's outstanding
 *     work; reset() is enqueued behind the previous call and ahead of the
 *     next.  Setters cannot be captured into a hipGraph; *_dev calls and
 *     reset() can, once the handle's tables are uploaded (its first call
 *     after a setter) and on the stream of the handle's previous call.
 *     A handle with carried state (pcx_freqdemod, pcx_fmchain) keeps it in
 *     two device slots it alternates between, and a captured call replays
 *     with the slots it was captured with: capture reset() in front of the
 *     calls (every replay starts a new stream), or an EVEN number of calls
 *     per handle (every replay continues where the previous one ended).
 *   - the library reads no environment variable.
 *   - input and output buffers of one call must not overlap, with two exceptions the reference
 *     relies on or that cost nothing: the same-size element-wise maps (rotate, scale, conj, arith and the pcx_bitwise* / pcx_bitshift /
 *     pcx_byteswap / pcx_arith_const / pcx_mathfn family, whose other overlaps are refused with PCX_ERR_ARG)
 *     accept out == in exactly (Arithmetic forwards input 0's buffer, Arithmetic.cpp:157-158), and
 *     the FFT accepts out == in.  abs/angle (narrower output), FIR, FreqDemod and the fused chain
 *     read what another lane may already have overwritten: no aliasing.
 *   - there is NO CPU fallback: a type/size the device path does not implement
 *     returns PCX_ERR_UNSUPPORTED.  After round 3 nothing of the path does: every numBins the reference
 *     constructs has a plan for every type FFTFactory accepts (complex_int16 beyond one workgroup's LDS runs
 *     kf_work's stages one launch each, bit-exact; transforms beyond 2^26 bins are refused), the FIR's
 *     PCX_FIR_OLS_FFT request is refused only for geometries it does not cover (PCX_FIR_AUTO always runs).
 */
#ifndef PCX_H
#define PCX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCX_API __attribute__((visibility("default")))

typedef enum pcx_scalar {
    PCX_F64 = 0, PCX_F32 = 1, PCX_I64 = 2, PCX_I32 = 3, PCX_I16 = 4, PCX_I8 = 5,
    /* unsigned element types: accepted by pcx_arith*, pcx_arith_const*, pcx_compare*, pcx_bitwise* and pcx_bitshift* only
     * (arithmeticFactory, Arithmetic.cpp:284-296, and the factories of the blocks those calls serve) */
    PCX_U64 = 6, PCX_U32 = 7, PCX_U16 = 8, PCX_U8 = 9
} pcx_scalar;

typedef enum pcx_status {
    PCX_OK = 0,
    PCX_ERR_ARG = -1,          /* Pothos::InvalidArgumentException territory */
    PCX_ERR_UNSUPPORTED = -2,  /* valid in the reference, not implemented on device */
    PCX_ERR_HIP = -3,          /* a HIP runtime call failed */
    PCX_ERR_STATE = -4         /* call sequence error (e.g. process before taps upload) */
} pcx_status;

PCX_API const char *pcx_last_error(void);
PCX_API const char *pcx_version(void);

/* ---- Pothos::Util::floatToQ / fromQ for INTEGER element types --------------------------------------------------------------
 * Call sites in the reference: filter/FIRFilter.cpp:300 (fromQ<OutType>(y_n)) and :348 (floatToQ<QTapsType>(taps)),
 * math/Rotate.cpp:21,74, math/Scale.cpp:21,73.  The header that defines them, PothosCore's include/Pothos/Util/QFormat.hpp, is
 * NOT under /root/reference (CMakeLists.txt:8 only names the package), and the reference tests that go through it
 * (math/TestRotate.cpp:53, math/TestScale.cpp:52: multiples of 10 times 0, +-0.5, +-1, tolerance 1) leave TWELVE readings
 * standing (profiles/r02/qformat_enumeration.txt):
 *     fractional bits n     half the Q word (PCX_Q_FRAC_HALF_Q)    |  half the ELEMENT word (PCX_Q_FRAC_HALF_ELEM)
 *     floatToQ<T>(x)        T(ldexp(x, n)), the cast truncating    |  rounding to nearest (ties away from zero)
 *     fromQ<T>(q)           q >> n (floor)  |  q / 2^n (toward zero)  |  (q + 2^(n-1)) >> n (nearest, ties up)
 * with Q the widened accumulator type of the factories (int8 -> int16, int16 -> int32, int32 -> int64, int64 -> int64:
 * FIRFilter.cpp:377-382, Rotate.cpp:143-157, Scale.cpp:142-157).  Every integer FIR, Rotate and Scale path of this library takes
 * the reading as a parameter; the all-zero pcx_qformat -- HALF_Q, TRUNCATE, FLOOR, the builder's recollection of the header -- is the
 * built-in default (kDefaultQFormat, csrc/pcx_internal.hpp: the ONE line to change the day the header is read).  Products and sums
 * wrap modulo 2^bits(Q) under every reading (std::complex<intN> arithmetic), the result of fromQ is truncated to the element
 * width.  Floating-point element types are not affected: both functions are plain casts there. */
typedef enum pcx_q_frac { PCX_Q_FRAC_HALF_Q = 0, PCX_Q_FRAC_HALF_ELEM = 1 } pcx_q_frac;
typedef enum pcx_q_to { PCX_Q_TRUNCATE = 0, PCX_Q_NEAREST = 1 } pcx_q_to;
typedef enum pcx_q_from { PCX_Q_FLOOR = 0, PCX_Q_TOWARD_ZERO = 1, PCX_Q_ROUND = 2 } pcx_q_from;
typedef struct pcx_qformat {
    int frac;          /* pcx_q_frac */
    int float_to_q;    /* pcx_q_to */
    int from_q;        /* pcx_q_from */
} pcx_qformat;
/* the process-wide reading: what handles created AFTERWARDS start with and what the stateless pcx_rotate* / pcx_scale* use.
 * NULL restores the built-in default.  Not synchronised with running calls: set it before the blocks are made. */
PCX_API int pcx_set_qformat(const pcx_qformat *q);
PCX_API int pcx_get_qformat(pcx_qformat *q);

/* ---- device plumbing (for hosts without their own HIP runtime binding) ---- */
PCX_API int pcx_device_count(int *count);
PCX_API int pcx_set_device(int ordinal);
PCX_API int pcx_get_device(int *ordinal);   /* the calling thread's current device */
PCX_API int pcx_dev_alloc(void **dptr, size_t bytes);
PCX_API int pcx_dev_free(void *dptr);
PCX_API int pcx_memcpy_h2d(void *dst_dev, const void *src_host, size_t bytes, void *stream);
PCX_API int pcx_memcpy_d2h(void *dst_host, const void *src_dev, size_t bytes, void *stream);
PCX_API int pcx_memcpy_d2d(void *dst_dev, const void *src_dev, size_t bytes, void *stream);
/* what kind of memory a buffer lives in -- a block's port buffer may be pageable host memory, one of the page-locked slabs of
 * pcx_host_alloc, or (an edge between two blocks of this module) device memory the CPU must not touch */
typedef enum pcx_pointer_kind_t { PCX_PTR_PAGEABLE = 0, PCX_PTR_PAGE_LOCKED = 1, PCX_PTR_DEVICE = 2 } pcx_pointer_kind_t;
PCX_API int pcx_pointer_kind(const void *p, int *kind);
/* bytes of `src` -- any of the three kinds -- into ordinary host memory, complete on return (FIRFilter::work's burst flush,
 * FIRFilter.cpp:263-272, builds its zero-padded tail on the host) */
PCX_API int pcx_memcpy_to_host(void *dst_host, const void *src, size_t bytes);
PCX_API int pcx_stream_sync(void *stream);
/* ROCTx ranges around every data-plane entry point (pcx_*_process[_dev], pcx_fft_transform[_dev], the maps,
 * pcx_shard_scatter/step/gather), named after the function: `rocprofv3 --marker-trace --kernel-trace` then shows which
 * call each kernel belongs to.  Off by default; pcx_trace(1) loads the ROCTx library (librocprofiler-sdk-roctx.so.1,
 * else libroctx64.so.4) and returns PCX_ERR_UNSUPPORTED when there is none; pcx_trace(0) switches the ranges off.
 * Process-wide. */
PCX_API int pcx_trace(int on);
/* page-locked host memory for port buffers: a Pothos BufferManager that hands out slabs from
 * pcx_host_alloc lets the plain (host-pointer) entry points copy at PCIe line rate instead of
 * staging pageable memory */
PCX_API int pcx_host_alloc(void **hptr, size_t bytes);
PCX_API int pcx_host_free(void *hptr);
/* Page-lock memory the FRAMEWORK owns, where it lies (hipHostRegister, portable + mapped): afterwards the host-pointer entry points
 * treat it like a pcx_host_alloc slab (in place over PCIe, nothing staged).  The FIR's input inside Pothos is such memory: the
 * reference asks the framework for its "circular" manager (filter/FIRFilter.cpp:196-199), whose buffer is pageable and mapped twice
 * back to back so that a window may run across the wrap.
 *   pcx_host_register(ptr, bytes)    [ptr, ptr + bytes), page-aligned by the caller.  Memory that is already page-locked is PCX_OK.
 *   pcx_host_unregister(ptr)         the range registered at ptr (a range this library did not register: PCX_ERR_ARG).
 *   pcx_host_register_mapping(p, bytes, max_bytes, &base, &len)
 *                                    finds the mapping(s) of this process that hold [p, p + bytes) (/proc/self/maps), widens the range
 *                                    over ADJACENT mappings of the same shared file object -- the two halves of a double-mapped
 *                                    circular buffer are one object mapped twice -- and page-locks all of it; *base / *len say what
 *                                    was locked (pass *base to pcx_host_unregister).  A range beyond max_bytes (0: 1 GiB), memory that
 *                                    is not a shared mapping (a heap arena, a stack: locking one would pin whatever else lives
 *                                    there) and memory somebody else page-locked leave *base NULL and return PCX_OK: nothing to undo.
 * Registrations are COUNTED: a range this library holds already (two blocks on one buffer, one block under a second window)
 * gets one more holder and the same *base / *len, and pcx_host_unregister only unlocks when the last holder has let go.
 *   pcx_host_mapping_alive(base, &alive)
 *                                    is what was mapped at base when it was locked (device and inode of the shared object, the whole
 *                                    range, read-write) still mapped there?  The lock belongs to the MAPPING: after the framework has
 *                                    unmapped a buffer, a new one at the same address is not page-locked, whatever the old entry says.
 *                                    A holder asks when its block is activated, and lets go of what is no longer alive.
 *   pcx_host_release_range(p, bytes) for the OWNER of the memory, in front of munmap: every registration of this library that overlaps
 *                                    [p, p + bytes) is dropped, whoever holds it, and unlocked.
 * The /comms/fir_filter block calls pcx_host_register_mapping the first time it sees a pageable port buffer and whenever the
 * buffer's address leaves what it has locked; it lets go in deactivate() (a topology that is re-committed re-allocates its buffers
 * between deactivate and activate) and in its destructor, and checks what it still holds in activate(). */
PCX_API int pcx_host_register(void *ptr, size_t bytes);
PCX_API int pcx_host_unregister(void *ptr);
PCX_API int pcx_host_register_mapping(const void *p, size_t bytes, size_t max_bytes, void **base, size_t *len);
PCX_API int pcx_host_mapping_alive(const void *base, int *alive);
PCX_API int pcx_host_release_range(const void *p, size_t bytes);
/* synthetic stream generator on the device: the same splitmix64 counter hash as
 * the oracle's orc_fill_uniform_f32 (uniform [-1,1), bit-identical values) */
PCX_API int pcx_fill_uniform_f32_dev(float *dst_dev, size_t n_scalars, uint64_t seed, uint64_t offset, void *stream);
/* measurement aid (no reference counterpart): the PCIe roof of this box as the copy engines see it.  `bytes` of page-locked host
 * memory each way, `reps` transfers queued back to back behind a warm-up one: host -> device alone, device -> host alone, and BOTH at
 * once on two streams of the probe's own -- GB/s per direction.  bench.py prices the host-pointer path (secondary.host_path, bound "pcie") on the
 * FASTER of the two directions alone (the link is full duplex: what one direction carries alone is the ceiling of each; *both_gbs is
 * reported beside it, it depends on which HIP runtime the process loaded), measured in the same run.  Allocates and frees 2 x bytes
 * of host and of device memory; blocks until done. */
PCX_API int pcx_pcie_probe(size_t bytes, int reps, double *h2d_gbs, double *d2h_gbs, double *both_gbs);
/* measurement aid (no reference counterpart): ONE wave on `stream` spins for spin_us microseconds and writes the shader clock it
 * ran at, in MHz, to *mhz_dev (shader cycles from s_memtime over the 100 MHz s_memrealtime).  Queued on a stream of its own beside
 * a running workload it reads the clock the workload is held at by the package power cap -- bench.py uses it to turn the profiled
 * VALU instruction count of a kernel into a share of SIMD issue time (`roofline.valu`). */
PCX_API int pcx_clock_probe_dev(float *mhz_dev, unsigned spin_us, void *stream);

/* ===================================================================== *
 *  /comms/fir_filter      filter/FIRFilter.cpp
 * ===================================================================== */
typedef struct pcx_fir pcx_fir;

typedef enum pcx_fir_algo {
    PCX_FIR_AUTO = 0,    /* OLS_FFT when it applies and pays, else DIRECT */
    PCX_FIR_DIRECT = 1,  /* time-domain LDS-tiled dot product (FMA) */
    PCX_FIR_OLS_FFT = 2, /* frequency-domain overlap-save on 4096-sample blocks: complex_float32 (K <= 8193 -- beyond
                            2049 taps the taps in partitions of 2048 against the previous windows' spectra, decimating
                            and interpolating filters as well, K per polyphase row), real float32 (K <= 8193, likewise),
                            complex_float64 and M = L = 1 (K <= 4097), complex_int16 / complex_int8 and real float64 / int16 / int8 with
                            M = L = 1 (K <= 4097; integers bit-exact: the rounded double-precision sums are the integer
                            convolution); anything else -> PCX_ERR_UNSUPPORTED */
    PCX_FIR_EXACT = 3    /* time-domain, reference accumulation order, no FMA:
                            bit-identical to FIRFilter.cpp:295-300 for float types */
} pcx_fir_algo;

/* FIRFilterFactory(dtype, tapsType), FIRFilter.cpp:369-384.
 * complex_taps = 1 is tapsType "COMPLEX" (complex element types only). */
PCX_API int pcx_fir_create(int scalar, int is_complex, int complex_taps, pcx_fir **out);
PCX_API int pcx_fir_destroy(pcx_fir *h);
/* setTaps, FIRFilter.cpp:138-144 + updateInternals :327-354.  `taps` holds ntaps
 * doubles (REAL) or ntaps (re,im) double pairs (COMPLEX).  ntaps == 0 -> PCX_ERR_ARG. */
PCX_API int pcx_fir_set_taps(pcx_fir *h, const double *taps, size_t ntaps);
/* setDecimation / setInterpolation, FIRFilter.cpp:151-168.  0 -> PCX_ERR_ARG. */
PCX_API int pcx_fir_set_decimation(pcx_fir *h, size_t decim);
PCX_API int pcx_fir_set_interpolation(pcx_fir *h, size_t interp);
PCX_API int pcx_fir_set_algo(pcx_fir *h, int algo);
/* the Q-format reading of THIS filter (integer element types; see pcx_qformat): the taps are quantised again with it and every
 * later call shifts and rounds by it.  NULL: the process-wide reading of pcx_set_qformat. */
PCX_API int pcx_fir_set_qformat(pcx_fir *h, const pcx_qformat *q);
/* K = ceil(ntaps/L) (FIRFilter.cpp:335) and _inputRequire = M+K-1 (:353) */
PCX_API int pcx_fir_get_geometry(const pcx_fir *h, size_t *K, size_t *input_require);
/* which algorithm the last process call ran (pcx_fir_algo) */
PCX_API int pcx_fir_last_algo(const pcx_fir *h);
/* pcx_fir_get_last_plan: which plan the last process call ran -- one value per branch of the choice pcx_fir_process_dev makes from the
 * handle's tables (pcx_fir_last_algo has three values; most plans report PCX_FIR_OLS_FFT).  NONE: no call has run yet.  A name says
 * which kernel ran and on which table layout: branches that launch one kernel with different tables have names of their own.
 *   CF32_OLS4096 / _GATED  complex_float32, M = L = 1, K <= 2049: the 4096-sample kernel; _GATED its launch behind a gate word
 *   CF32_UPOLS             the same stream, 2049 < K <= 8193: the partitioned kernel
 *   CF32_DECIM / _INTERP   complex_float32, the spectrum folded (M = 2 or 4- / 8- / 16-fold) / replicated (L in 2, 4, 8, 16)
 *   CF32_OLS4096_ROWS      complex_float32, M = 1, other L: every polyphase row through the 4096-sample kernel, then interleaved
 *   CF32_POLY              complex_float32, other (L, M): the polyphase kernel with strided stores
 *   F32_OLS4096 / F32_UPOLS / F32_OLS4096_ROWS   real float32: two real blocks per transform; its halves side by side through the
 *                          partitioned kernel beyond 2049 taps; its polyphase rows (L > 1, rows of up to 2049 taps)
 *   UPOLS_ROWS / UPOLS_DECIM   float32 or complex_float32: polyphase rows of 2050 .. 8193 taps / decimators (complex beyond 2049
 *                          taps, real of any length) through the partitioned kernel
 *   CF64_OLS / CF64_OLS_ROWS   complex_float64, complex_int16, complex_int8 on the double pipeline; its polyphase rows (L > 1)
 *   REAL64_OLS / REAL64_OLS_ROWS   real float64, int16, int8: two real blocks per double transform; its polyphase rows
 *   CF32_DIRECT_TILE       the LDS-tiled time-domain kernel (complex_float32, M = L = 1)
 *   DOT2 / SLIDE / GENERIC the time-domain kernels of every type: packed 16-bit dot products (complex_int16 / complex_int8, M = L = 1),
 *                          the sliding window (M = L = 1), one output per lane (any L, M)
 * It makes no device call. */
enum { PCX_FIR_PLAN_NONE = 0, PCX_FIR_PLAN_CF32_OLS4096 = 1, PCX_FIR_PLAN_CF32_OLS4096_GATED = 2, PCX_FIR_PLAN_CF32_UPOLS = 3,
       PCX_FIR_PLAN_CF32_DECIM = 4, PCX_FIR_PLAN_CF32_INTERP = 5, PCX_FIR_PLAN_CF32_OLS4096_ROWS = 6, PCX_FIR_PLAN_CF32_POLY = 7,
       PCX_FIR_PLAN_F32_OLS4096 = 8, PCX_FIR_PLAN_F32_UPOLS = 9, PCX_FIR_PLAN_F32_OLS4096_ROWS = 10, PCX_FIR_PLAN_UPOLS_ROWS = 11,
       PCX_FIR_PLAN_UPOLS_DECIM = 12, PCX_FIR_PLAN_CF64_OLS = 13, PCX_FIR_PLAN_CF64_OLS_ROWS = 14, PCX_FIR_PLAN_REAL64_OLS = 15,
       PCX_FIR_PLAN_REAL64_OLS_ROWS = 16, PCX_FIR_PLAN_CF32_DIRECT_TILE = 17, PCX_FIR_PLAN_DOT2 = 18, PCX_FIR_PLAN_SLIDE = 19,
       PCX_FIR_PLAN_GENERIC = 20 };
PCX_API int pcx_fir_get_last_plan(const pcx_fir *h, int *plan);
/* How many of the device's 1024 resident workgroup slots the handle's persistent launches may take (a multiple of 128; default
 * 1024 = the whole device).  For handles that run SIDE BY SIDE on one device -- several shards of a stream on one GPU, two filter
 * blocks of one topology -- so that their launches share the device instead of queueing behind one another's workgroups
 * (two 32 Mi-sample launches: 0.2196 ms with 1024 each, 0.1988 with 512 each; one 64 Mi launch 0.1971). */
PCX_API int pcx_fir_set_slots(pcx_fir *h, unsigned slots);
/*
 * The filter loop, FIRFilter.cpp:278-308.  `in` points at the front of the input
 * buffer: in_elems elements of which the first K-1 are history (the reference's
 * `x = in + (K-1)`, :281).  out_cap = room in the output buffer, in elements.
 *   N         = min((in_elems-(K-1))/M, out_cap/L)*M          (:278)
 *   *consumed = N                                              (:307)
 *   *produced = (N/M)*L                                        (:308)
 * Burst flush (:263-272) is the caller's job: it passes the zero-padded buffer.
 */
PCX_API int pcx_fir_process(pcx_fir *h, const void *in, size_t in_elems, void *out, size_t out_cap,
                            size_t *consumed, size_t *produced);
PCX_API int pcx_fir_process_dev(pcx_fir *h, const void *in_dev, size_t in_elems, void *out_dev, size_t out_cap,
                                size_t *consumed, size_t *produced, void *stream);
/*
 * The same call over ONE SHARD of a stream that is split across devices: the first K-1 samples of `in_dev` -- the
 * history slot, FIRFilter.cpp:281,305-307 -- are the HALO, still on its way from the left neighbour when the call is queued.
 * ONE launch covers the whole shard: the blocks at the front, the only ones that read the halo, are computed last and not before
 * the 32-bit word *gate_dev has reached gate_value (signed distance, so a pass counter needs no reset).  The caller queues
 * pcx_gate_signal_dev(gate_dev, gate_value, s) on the stream that carries the halo, behind the transfer; everything else of the
 * shard is filtered while the halo is in flight.
  * The wait is bounded: after two seconds without the signal the held blocks run on whatever the halo slot holds and the word
 * behind the gate word (gate_dev[1]) is set to 0xDEAD -- a gate takes two 32-bit words.
 * ORDER OF QUEUEING.  Queue the transfer and the signal BEFORE this call (pcx_shard_step and the RCCL driver do): then nothing the
 * gate waits for can sit behind the gated launch.  A signal queued AFTER it must not share the launch's HARDWARE queue -- HIP
 * maps a process's streams onto four of them, round robin, and a packet waits for every earlier packet of its queue whatever
 * stream it came from: a signal behind the launch in the same queue waits for the launch, which waits for the signal (measured:
 * every fourth stream a process creates times out, tools/gate_queue_probe.py).  A stream of ANOTHER PRIORITY
 * (hipStreamCreateWithPriority) has queues of its own: use one for a signal that has to be queued late -- or put the gate words
 * in page-locked host memory (hipHostMalloc; the waiting workgroup reads them in place with system-scope loads) and open the gate
 * from the host with a plain 32-bit store, as the host-driven driver of pothoscomms_amd/stream.py does.
 *   *gated = 1: queued as described.   *gated = 0: this configuration has no gated kernel (anything but complex_float32 with
 *   M = L = 1 and K <= 2049, or a call of fewer than ~2048 blocks) and NOTHING has been queued: the caller waits for the halo on
 *   `stream` itself (an event) and calls pcx_fir_process_dev.
 */
PCX_API int pcx_fir_process_dev_gated(pcx_fir *h, const void *in_dev, size_t in_elems, void *out_dev, size_t out_cap,
                                      size_t *consumed, size_t *produced, const void *gate_dev, unsigned gate_value, void *stream,
                                      int *gated);
/* a one-thread kernel on `stream`: *gate_dev <- value (system-scope release) */
PCX_API int pcx_gate_signal_dev(void *gate_dev, unsigned value, void *stream);

/* ===================================================================== *
 *  /comms/fft             fft/FFT.cpp, fft/FFTAux.h, fft/kissfft.hh, fft/kiss_fft.c
 * ===================================================================== */
typedef struct pcx_fft pcx_fft;
/* FFTFactory(dtype, numBins, inverse), FFT.cpp:83-93: scalar in {F64, F32, I16}
 * (always complex).  Forward = exp(-j..), inverse = exp(+j..), float paths
 * unscaled (kissfft.hh:81-161), int16 path scaled by 1/radix per stage
 * (kiss_fft.c:61, _kiss_fft_guts.h:73-78). */
PCX_API int pcx_fft_create(int scalar, size_t num_bins, int inverse, pcx_fft **out);
PCX_API int pcx_fft_destroy(pcx_fft *h);
/* FFTAux::transform over `nframes` back-to-back frames (FFT::work does one,
 * FFT.cpp:66-71; a device caller batches whole frames per call). */
PCX_API int pcx_fft_transform(pcx_fft *h, const void *in, void *out, size_t nframes);
PCX_API int pcx_fft_transform_dev(pcx_fft *h, const void *in_dev, void *out_dev, size_t nframes, void *stream);
/* pcx_fft_get_plan: which plan pcx_fft_create chose for (scalar, num_bins).  IDENTITY: one bin.  R16_4096 / R16 / POW2: one workgroup
 * per group of frames, radix 16 or radix 2 / 4 in LDS.  Q15_POW2 / Q15_GLOBAL: kiss_fft's Q15 stages in LDS / one launch per stage
 * over global memory.  MIXED: kissfft's factor order in LDS.  SMOOTH: 2^a 3^b 5^c bins, 16s first.  FOURSTEP / FOURSTEP_SHORT:
 * num_bins = n1 * n2 around two shorter plans / around the column and row kernels.  BLUESTEIN: chirp-z on power-of-two plans. */
enum { PCX_FFT_PLAN_IDENTITY = 0, PCX_FFT_PLAN_R16_4096 = 1, PCX_FFT_PLAN_R16 = 2, PCX_FFT_PLAN_POW2 = 3, PCX_FFT_PLAN_Q15_POW2 = 4,
       PCX_FFT_PLAN_Q15_GLOBAL = 5, PCX_FFT_PLAN_MIXED = 6, PCX_FFT_PLAN_SMOOTH = 7, PCX_FFT_PLAN_FOURSTEP = 8,
       PCX_FFT_PLAN_FOURSTEP_SHORT = 9, PCX_FFT_PLAN_BLUESTEIN = 10 };
/* *kind = the plan; *n1, *n2 = the split num_bins = n1 * n2 of the two four-step plans; for BLUESTEIN *n1 = num_bins and *n2 = M, the
 * power-of-two convolution size; 0 and 0 for every other plan.  Makes no device call. */
PCX_API int pcx_fft_get_plan(const pcx_fft *h, int *kind, size_t *n1, size_t *n2);

/* ===================================================================== *
 *  /comms/freq_demod      demod/FreqDemod.cpp
 * ===================================================================== */
typedef struct pcx_freqdemod pcx_freqdemod;
/* FreqDemodFactory(dtype), FreqDemod.cpp:80-93: complex<scalar> in, scalar out */
PCX_API int pcx_freqdemod_create(int scalar, pcx_freqdemod **out);
PCX_API int pcx_freqdemod_destroy(pcx_freqdemod *h);
/* activate(): _prev = 0, FreqDemod.cpp:44-47 */
PCX_API int pcx_freqdemod_reset(pcx_freqdemod *h);
/* the loop FreqDemod.cpp:60-67: out[i] = angle(in[i]*prev); prev = conj(in[i]);
 * prev is carried across calls inside the handle (device side) */
PCX_API int pcx_freqdemod_process(pcx_freqdemod *h, const void *in, void *out, size_t n);
PCX_API int pcx_freqdemod_process_dev(pcx_freqdemod *h, const void *in_dev, void *out_dev, size_t n, void *stream);

/* ===================================================================== *
 *  /comms/dc_removal      filter/DCRemoval.cpp, filter/MovingAverage.hpp
 * ===================================================================== */
typedef struct pcx_dcremoval pcx_dcremoval;
/* DCRemovalFactory(dtype), DCRemoval.cpp:121-136: scalar in {F64, F32, I64, I32, I16, I8}, real or complex; the accumulator types
 * are the reference's (f64, f32, i64, i64, i32, i16, complex alike).  Created at average size 512, cascade size 2. */
PCX_API int pcx_dcremoval_create(int scalar, int is_complex, pcx_dcremoval **out);
PCX_API int pcx_dcremoval_destroy(pcx_dcremoval *h);
/* setAverageSize / setCascadeSize (DCRemoval.cpp:57-79): zero -> PCX_ERR_ARG; every stage starts over.  The device state and
 * workspace are allocated here, never in a process call. */
PCX_API int pcx_dcremoval_set_sizes(pcx_dcremoval *h, size_t average_size, size_t cascade_size);
PCX_API int pcx_dcremoval_get_sizes(const pcx_dcremoval *h, size_t *average_size, size_t *cascade_size);
/* activate(): every stage's history and accumulator back to zero */
PCX_API int pcx_dcremoval_reset(pcx_dcremoval *h);
/* the loop DCRemoval.cpp:100-110 over n elements, state carried across calls.  Integer types are bit-exact with the reference
 * compiled for x86-64; float types are computed without the reference's drift (DESIGN.md 9 gives the bounds).  A divisor that the
 * accumulator type narrows to zero (the reference divides by zero there) -> PCX_ERR_ARG, nothing launched, out untouched: complex_int8
 * at average sizes that are multiples of 256, complex_int16 at multiples of 65536, int8 at multiples of 65536.  After a set_sizes that
 * failed to allocate, every call but set_sizes and destroy -> PCX_ERR_STATE. */
PCX_API int pcx_dcremoval_process(pcx_dcremoval *h, const void *in, void *out, size_t n);
PCX_API int pcx_dcremoval_process_dev(pcx_dcremoval *h, const void *in_dev, void *out_dev, size_t n, void *stream);

/* ===================================================================== *
 *  /comms/envelope_detector      filter/EnvelopeDetector.cpp
 * ===================================================================== */
typedef struct pcx_envelope pcx_envelope;
/* EnvelopeDetectorFactory(dtype), EnvelopeDetector.cpp:163-178: scalar in {F64, F32, I64, I32, I16, I8}, real or complex; the
 * output is float32 whatever the input.  Created as the reference constructs the block: every gain 0 (a handle whose setters were
 * never called outputs zeros), envelope 0, lookahead 0.  The device state and workspace are allocated here. */
PCX_API int pcx_envelope_create(int scalar, int is_complex, pcx_envelope **out);
PCX_API int pcx_envelope_destroy(pcx_envelope *h);
/* setAttack / setRelease (EnvelopeDetector.cpp:76-99): gain = std::exp(-1/t) and 1 - gain in float, on the host.  Neither resets
 * the envelope. */
PCX_API int pcx_envelope_set_attack(pcx_envelope *h, float attack);
PCX_API int pcx_envelope_get_attack(const pcx_envelope *h, float *attack);
PCX_API int pcx_envelope_set_release(pcx_envelope *h, float release);
PCX_API int pcx_envelope_get_release(const pcx_envelope *h, float *release);
PCX_API int pcx_envelope_set_lookahead(pcx_envelope *h, size_t lookahead);
PCX_API int pcx_envelope_get_lookahead(const pcx_envelope *h, size_t *lookahead);
/* the envelope back to 0 (for API users: the block never calls it, as the reference has no activate()) */
PCX_API int pcx_envelope_reset(pcx_envelope *h);
/* the carried envelope after the handle's last call (waits for that call) */
PCX_API int pcx_envelope_get_state(pcx_envelope *h, float *envelope);
/* work()'s loop (EnvelopeDetector.cpp:110-148) for n outputs: reads n + lookahead input elements from in, out[i] from in[i +
 * lookahead], writes n floats, carries the envelope.  Bit for bit the reference's float32 arithmetic (any NaN for a NaN).
 * process_dev synchronises nothing and allocates nothing: it can be captured into a graph. */
PCX_API int pcx_envelope_process(pcx_envelope *h, const void *in, void *out, size_t n);
PCX_API int pcx_envelope_process_dev(pcx_envelope *h, const void *in_dev, void *out_dev, size_t n, void *stream);
/* the last call's path counts (waits for that call): chunks computed speculatively, chunks whose repair pass rewrote outputs,
 * chunks the in-order resolve pass re-ran.  Slow time constants show up as repaired and resolved chunks. */
PCX_API int pcx_envelope_get_stats(pcx_envelope *h, uint64_t *chunks, uint64_t *repaired, uint64_t *resolved);
/* tuning: warm-up samples in front of each speculative chunk; 0 (the default) derives it from the gains */
PCX_API int pcx_envelope_set_warmup(pcx_envelope *h, size_t warmup);

/* ===================================================================== *
 *  /comms/iir_filter      filter/IIRFilter.cpp
 * ===================================================================== */
typedef struct pcx_iir pcx_iir;
/* pcx_iir_get_plan: how a configured handle computes */
enum { PCX_IIR_SCAN = 0, PCX_IIR_SERIAL = 1 };
/* IIRFilterFactory(dtype), IIRFilter.cpp:107-121: scalar in {F64, F32, I64, I32, I16, I8}, real or complex (two independent real
 * recurrences).  Created with the reference's default taps [0.0676, 0.135, 0.0676, 1, -1.142, 0.412] and a zero history.  The device
 * state and workspace are allocated here, for every order and one slice. */
PCX_API int pcx_iir_create(int scalar, int is_complex, pcx_iir **out);
PCX_API int pcx_iir_destroy(pcx_iir *h);
/* setTaps (IIRFilter.cpp:63-69): b[0..N] then a[0..N], 1 <= N + 1 <= 33, normalised by a[0] in double.  PCX_ERR_ARG, checked before
 * the handle: no taps, an odd count, more than 66, a non-finite tap, a[0] == 0.  Chooses the plan (Schur-Cohn: SCAN for a stable
 * filter, SERIAL otherwise) and zeroes the history. */
PCX_API int pcx_iir_set_taps(pcx_iir *h, const double *taps, size_t n);
/* the taps as last set: *n = their count, at most cap of them copied */
PCX_API int pcx_iir_get_taps(const pcx_iir *h, double *taps, size_t cap, size_t *n);
/* activate(): the history back to zero */
PCX_API int pcx_iir_reset(pcx_iir *h);
/* the plan, and for SCAN the a-priori bound: every output before narrowing lies within bound * max|x| of the sequential double
 * recurrence's value (0 for SERIAL, which is that recurrence bit for bit) */
PCX_API int pcx_iir_get_plan(const pcx_iir *h, int *plan, double *bound);
/* work()'s loop (IIRFilter.cpp:82-99) over n elements, the history carried across calls: y = sum b_k x[n-k] - sum a_k y[n-k] in
 * double, narrowed to the stream type (float32 to nearest; integers toward zero, saturated, NaN -> 0).  Checked in this order before
 * any device call: the handle, n == 0 (nothing to do), null buffers, any overlap of the n input elements with the n output elements
 * (PCX_ERR_ARG, out == in included: the kernels read a slice's inputs again after outputs have been written).  process_dev
 * synchronises nothing and allocates nothing: it can be captured into a graph. */
PCX_API int pcx_iir_process(pcx_iir *h, const void *in, void *out, size_t n);
PCX_API int pcx_iir_process_dev(pcx_iir *h, const void *in_dev, void *out_dev, size_t n, void *stream);

/* ===================================================================== *
 *  /comms/scrambler, /comms/descrambler      digital/Scrambler.cpp, digital/Descrambler.cpp, digital/lfsr.h
 *
 *  One unsigned char per bit in and out; only bit 0 of an input byte counts, an output byte is 0 or 1.  Every output bit and the
 *  register equal the reference's.
 * ===================================================================== */
typedef struct pcx_scrambler pcx_scrambler;
enum { PCX_SCR_ADDITIVE = 0, PCX_SCR_MULTIPLICATIVE = 1 };
/* pcx_scrambler_get_plan: how a configured handle computes */
enum { PCX_SCR_SCAN = 0, PCX_SCR_SERIAL = 1 };
/* the constructors (Scrambler.cpp:43-62, Descrambler.cpp:43-62): descramble = 0 the scrambler, otherwise the descrambler; multiplicative,
 * seed 1, setPoly(0x19).  The device state, tables and workspace of one slice are allocated here. */
PCX_API int pcx_scrambler_create(int descramble, pcx_scrambler **out);
PCX_API int pcx_scrambler_destroy(pcx_scrambler *h);
/* setPoly (Scrambler.cpp:64-68): GLFSR_init(poly, seed), lfsr.h:63-83 -- polynomial = poly | 1, data = seed, mask = every bit from the
 * polynomial's top bit upward (the shift is arithmetic); the mask is KEPT when poly has no bit in 63..1.  Chooses the plan: SCAN when
 * the polynomial owns the mask's lowest bit m and 0 <= seed < 2^m, SERIAL otherwise. */
PCX_API int pcx_scrambler_set_poly(pcx_scrambler *h, int64_t poly);
PCX_API int pcx_scrambler_get_poly(const pcx_scrambler *h, int64_t *poly);
/* setSeed (Scrambler.cpp:75-79): GLFSR_init(poly, seed) as above */
PCX_API int pcx_scrambler_set_seed(pcx_scrambler *h, int64_t seed);
PCX_API int pcx_scrambler_get_seed(const pcx_scrambler *h, int64_t *seed);
/* setMode (Scrambler.cpp:86-91): PCX_SCR_ADDITIVE or PCX_SCR_MULTIPLICATIVE, anything else PCX_ERR_ARG (checked before the handle);
 * the register is left alone */
PCX_API int pcx_scrambler_set_mode(pcx_scrambler *h, int mode);
PCX_API int pcx_scrambler_get_mode(const pcx_scrambler *h, int *mode);
PCX_API int pcx_scrambler_get_plan(const pcx_scrambler *h, int *plan);
/* bits a thread, a tile, a wave of the carry and a slice of the SCAN plan hold (the seams a test wants to straddle) */
PCX_API int pcx_scrambler_get_geometry(size_t *run, size_t *tile, size_t *group, size_t *slice);
/* lfsr_t's data and mask after the handle's last call (waits for it) */
PCX_API int pcx_scrambler_get_state(pcx_scrambler *h, int64_t *data, int64_t *mask);
/* work()'s loop (Scrambler.cpp:154-181, Descrambler.cpp:154-181) over n bytes, the register carried across calls.  out may be in
 * itself (in place); any other overlap of the two is PCX_ERR_ARG.  process_dev synchronises nothing and allocates nothing: it can
 * be captured into a graph. */
PCX_API int pcx_scrambler_process(pcx_scrambler *h, const void *in, void *out, size_t n);
PCX_API int pcx_scrambler_process_dev(pcx_scrambler *h, const void *in_dev, void *out_dev, size_t n, void *stream);

/* ===================================================================== *
 *  /comms/preamble_correlator      digital/PreambleCorrelator.cpp
 *
 *  One unsigned char per symbol.  For every position n < n_in - P the Hamming distance over whole bytes,
 *  dist[n] = sum over i < P of popcount(preamble[i] ^ in[n + i]) (:134-143): the upper bits of an input byte count.  A position
 *  with dist <= threshold is a match and its label index is n + P (:145-148), which may lie up to P - 1 past the last position.
 *  Every index, count and distance equals the reference's.  Nothing is carried from one call to the next.
 * ===================================================================== */
typedef struct pcx_preamble pcx_preamble;
/* pcx_preamble_get_plan: how a configured handle computes the distances -- per bit plane of the symbols (preambles of up to
 * max_planes_len symbols, pcx_preamble_get_geometry), or the reference's byte loop, one position per thread (longer ones) */
enum { PCX_PRE_PLANES = 0, PCX_PRE_BYTES = 1 };
/* the constructor (:60-75): preamble {1}, threshold 1.  Where a device can be reached the workspace of one slice is allocated and
 * the packed preamble uploaded here and in set_preamble; otherwise at the first call that computes. */
PCX_API int pcx_preamble_create(pcx_preamble **out);
PCX_API int pcx_preamble_destroy(pcx_preamble *h);
/* setPreamble (:77-81): n == 0 is PCX_ERR_ARG "preamble cannot be empty" */
PCX_API int pcx_preamble_set_preamble(pcx_preamble *h, const unsigned char *symbols, size_t n);
/* *n = the preamble's length; the first min(*n, cap) symbols go to out (out may be NULL when cap is 0) */
PCX_API int pcx_preamble_get_preamble(const pcx_preamble *h, unsigned char *out, size_t cap, size_t *n);
PCX_API int pcx_preamble_set_threshold(pcx_preamble *h, unsigned threshold);
PCX_API int pcx_preamble_get_threshold(const pcx_preamble *h, unsigned *threshold);
PCX_API int pcx_preamble_get_plan(const pcx_preamble *h, int *plan);
/* positions a workgroup and a call slice hold (the seams a test wants to straddle), and the longest preamble of the PLANES plan */
PCX_API int pcx_preamble_get_geometry(size_t *tile, size_t *slice, size_t *max_planes_len);
/* work() (:114-154) on in[0 .. n_in): *n_positions = n_in > P ? n_in - P : 0; idx receives the label indices n + P in ascending
 * order, the first min(*n_matches, idx_cap) of them; *n_matches is always the full count.  out, when not NULL, receives the first
 * *n_positions input bytes (out == in is allowed, any other overlap is PCX_ERR_ARG).  Checked in this order before any device
 * call: the handle, the two counts.  process_dev takes device pointers throughout, the two counts included, allocates nothing
 * and synchronises nothing: it can be captured into a graph. */
PCX_API int pcx_preamble_process(pcx_preamble *h, const void *in, size_t n_in, void *out, uint64_t *idx, size_t idx_cap, size_t *n_positions,
                                 size_t *n_matches);
PCX_API int pcx_preamble_process_dev(pcx_preamble *h, const void *in_dev, size_t n_in, void *out_dev, uint64_t *idx_dev, size_t idx_cap,
                                     uint64_t *n_positions_dev, uint64_t *n_matches_dev, void *stream);
/* dist[n] for every position (the reference's commented-out second port, :65, :133, :150): dist holds n_in - P words */
PCX_API int pcx_preamble_distances(pcx_preamble *h, const void *in, size_t n_in, uint32_t *dist, size_t *n_positions);
PCX_API int pcx_preamble_distances_dev(pcx_preamble *h, const void *in_dev, size_t n_in, uint32_t *dist_dev, void *stream);

/* ===================================================================== *
 *  /comms/threshold      utility/Threshold.cpp
 *
 *  A real stream against two levels, one bit of carried state (:130-144): an inactive block turns active at an element
 *  x > activation, otherwise an active one turns inactive at x < deactivation.  Every label of the reference marks such a change,
 *  so the two kinds alternate: a call returns ONE ascending list of transition indices and the state in which it was entered, and
 *  transition j is an activation exactly when (entry state + j) is even.  The comparisons are the element type's own (a NaN
 *  element or level compares false, int64 never passes through double): every index equals the reference's.
 * ===================================================================== */
typedef struct pcx_threshold pcx_threshold;
/* ThresholdFactory (:163-174): scalar in {F64, F32, I64, I32, I16, I8}, anything else is PCX_ERR_ARG.  Both levels 0, inactive
 * (:54-58).  Where a device can be reached the workspace of one slice is allocated here; otherwise at the first call that computes. */
PCX_API int pcx_threshold_create(pcx_threshold **out, int scalar);
PCX_API int pcx_threshold_destroy(pcx_threshold *h);
/* each pointer addresses ONE ELEMENT of the handle's type (an int64 level keeps its 64 bits) */
PCX_API int pcx_threshold_set_levels(pcx_threshold *h, const void *activation, const void *deactivation);
PCX_API int pcx_threshold_get_levels(const pcx_threshold *h, void *activation, void *deactivation);
/* activate() (:111-115): inactive again.  get_state / set_state read and write the carried state (0 inactive, else active).
 * All three wait for what the handle has in flight. */
PCX_API int pcx_threshold_reset(pcx_threshold *h);
PCX_API int pcx_threshold_get_state(pcx_threshold *h, int *active);
PCX_API int pcx_threshold_set_state(pcx_threshold *h, int active);
/* elements a workgroup and a call slice hold (the seams a test wants to straddle) */
PCX_API int pcx_threshold_get_geometry(size_t *tile, size_t *slice);
/* work() (:117-149) on in[0 .. n): idx receives the indices of the elements at which the state changed, ascending, the first
 * min(*n_transitions, idx_cap) of them; *n_transitions is always the full count, *state_in the state the call was entered in; the
 * carried state advances whatever idx_cap is.  out, when not NULL, receives the n elements (out == in is allowed, any other overlap
 * is PCX_ERR_ARG).  n == 0 stores nothing, leaves the state alone and reports (0, the state).  Checked in this order before any
 * device call: the handle, the counts, in, idx_cap without idx, the overlap.  process_dev takes device pointers throughout;
 * counts_dev receives three words: n, the transitions, the entry state.  It allocates nothing and synchronises nothing: it can be
 * captured into a graph. */
PCX_API int pcx_threshold_process(pcx_threshold *h, const void *in, size_t n, void *out, uint64_t *idx, size_t idx_cap, size_t *n_transitions,
                                  int *state_in);
PCX_API int pcx_threshold_process_dev(pcx_threshold *h, const void *in_dev, size_t n, void *out_dev, uint64_t *idx_dev, size_t idx_cap,
                                      uint64_t *counts_dev, void *stream);
/* the state AFTER every element, one byte each (0 / 1), entered in the carried state -- which these two calls leave as it is */
PCX_API int pcx_threshold_states(pcx_threshold *h, const void *in, size_t n, unsigned char *states);
PCX_API int pcx_threshold_states_dev(pcx_threshold *h, const void *in_dev, size_t n, unsigned char *states_dev, void *stream);

/* ===================================================================== *
 *  /comms/signal_probe      utility/SignalProbe.cpp
 *
 *  One number from a window of the stream (:123-163): the last element (VALUE, :141), sqrt(sum |x|^2 / N) (RMS, :142-153) or
 *  sum x / N (MEAN, :154-160), with every element converted to double resp. std::complex<double> first.  A value is a PAIR of doubles
 *  (re, im); im is 0 for a real stream and for RMS.  The reference adds in stream order; the device adds over one fixed tree that
 *  depends on the element type and the window's length alone, so a window's pair is the same bit for bit at any byte
 *  address, anywhere in a batch and from run to run, and within (ceil(log2 N) + 2) u sum |x| / N of the exact mean resp.
 *  (ceil(log2 N) + 6) u of the exact RMS, u = 2^-53.  The rate limit, the mode strings and the signals are the block's (probe_blocks.cpp).
 * ===================================================================== */
typedef struct pcx_probe pcx_probe;
enum { PCX_PROBE_VALUE = 0, PCX_PROBE_RMS = 1, PCX_PROBE_MEAN = 2 };
/* signalProbeFactory (:176-188): scalar in {F64, F32, I64, I32, I16, I8}, real or complex; anything else is PCX_ERR_ARG "unsupported
 * type".  Mode VALUE, window 1024 (:64-67).  Where a device can be reached the scratch of the large-window path is allocated here,
 * once; otherwise at the first call that computes. */
PCX_API int pcx_probe_create(pcx_probe **out, int scalar, int is_complex);
PCX_API int pcx_probe_destroy(pcx_probe *h);
/* setMode / getMode (:87-95) for the three modes that calculate: any other code is PCX_ERR_ARG (a block keeps an unknown string itself) */
PCX_API int pcx_probe_set_mode(pcx_probe *h, int mode);
PCX_API int pcx_probe_get_mode(const pcx_probe *h, int *mode);
/* setWindow / getWindow (:97-106); 0 is PCX_ERR_ARG (the reference would read x[-1], :141) */
PCX_API int pcx_probe_set_window(pcx_probe *h, size_t window);
PCX_API int pcx_probe_get_window(const pcx_probe *h, size_t *window);
/* in elements of the handle's type: the longest window a workgroup reduces alone (up to a quarter of it a wave does), the slice
 * of a longer window that a workgroup reduces to a partial, and the shortest window that takes the large-window path (the seams a
 * test wants to straddle) */
PCX_API int pcx_probe_get_geometry(const pcx_probe *h, size_t *tile, size_t *slice, size_t *switch_over);
/* work() (:123-163) on in[0 .. n): N = min(window, n) elements are reduced, value_re_im receives the pair and *consumed = N.  With
 * N == 0 nothing is consumed and the pair is left as it is.  process takes host pointers (staged, or in place when page-locked) and
 * returns with the pair in host memory; process_dev takes device pointers, leaves the pair in device memory, allocates nothing and
 * synchronises nothing: it can be captured into a graph.  Checked in this order before any device call: the handle, consumed, the
 * pair, in. */
PCX_API int pcx_probe_process(pcx_probe *h, const void *in, size_t n, double *value_re_im, size_t *consumed);
PCX_API int pcx_probe_process_dev(pcx_probe *h, const void *in_dev, size_t n, double *value_re_im_dev, size_t *consumed, void *stream);
/* the batch: ceil(n / window) pairs, pair k what process returns for in[k window .. min((k + 1) window, n)), bit for bit */
PCX_API int pcx_probe_windows(pcx_probe *h, const void *in, size_t n, double *values);
PCX_API int pcx_probe_windows_dev(pcx_probe *h, const void *in_dev, size_t n, double *values_dev, void *stream);

/* ===================================================================== *
 *  /comms/wave_trigger      utility/WaveTrigger.cpp
 *
 *  The two device parts of the block: the level search (:735-771) and the capture of the windows (:515-582).  The search converts the
 *  stream to float -- static_cast<float> per component, a complex element to the modulus of its converted components, glibc's hypotf --
 *  and looks at the pairs (y[i], y[i + 1]): a pair triggers when y0 < level && y1 >= level (POS), y0 > level && y1 <= level (NEG) or
 *  either (LEVEL), compared in double.  It reports the LEAST triggering i and the pair's two floats; the caller forms the reference's
 *  position i + (level - y0) / (y1 - y0) from them (a float subtraction, the rest double), see pcx_trigger_position.  The result is a
 *  minimum: the same from run to run.  Modes, hold-off, windows, labels and messages are the block's (trigger_blocks.cpp).
 * ===================================================================== */
typedef struct pcx_trigger pcx_trigger;
enum { PCX_TRIGGER_POS = 0, PCX_TRIGGER_NEG = 1, PCX_TRIGGER_LEVEL = 2 };
#define PCX_TRIGGER_MAX_PORTS 16
/* what a search leaves: 24 bytes.  found is 0 or 1; with 0 the other three are 0 */
typedef struct pcx_trigger_hit {
    uint64_t i;
    float y0, y1;
    uint64_t found;
} pcx_trigger_hit;
/* scalar in {F64, F32, I64, I32, I16, I8}, real or complex, or {U64, U32, U16, U8}, real; anything else is PCX_ERR_ARG.  Level 0.5,
 * slope POS (:222-224) */
PCX_API int pcx_trigger_create(pcx_trigger **out, int scalar, int is_complex);
PCX_API int pcx_trigger_destroy(pcx_trigger *h);
PCX_API int pcx_trigger_set_level(pcx_trigger *h, double level);
PCX_API int pcx_trigger_get_level(const pcx_trigger *h, double *level);
/* PCX_TRIGGER_POS / NEG / LEVEL; any other code is PCX_ERR_ARG */
PCX_API int pcx_trigger_set_slope(pcx_trigger *h, int slope);
PCX_API int pcx_trigger_get_slope(const pcx_trigger *h, int *slope);
/* the pairs a workgroup searches at a time (the seam a test wants to straddle) */
PCX_API int pcx_trigger_get_geometry(const pcx_trigger *h, size_t *tile);
/* the least triggering pair i with from <= i <= n - 2 of the n elements at in (none when n < 2 or from > n - 2).  search takes a host
 * pointer (pageable: staged; page-locked or device memory: searched where it lies) and returns the hit; only the 24 bytes of the
 * result are read back.  search_dev takes device pointers, leaves the hit in device memory, allocates nothing and synchronises
 * nothing.  Checked in this order before any device call: the handle, the hit, in. */
PCX_API int pcx_trigger_search(pcx_trigger *h, const void *in, size_t n, size_t from, pcx_trigger_hit *hit);
PCX_API int pcx_trigger_search_dev(pcx_trigger *h, const void *in_dev, size_t n, size_t from, pcx_trigger_hit *hit_dev, void *stream);
/* searchTriggerPointReal's result from a hit (:747): i + (level - y0) / (y1 - y0), y1 - y0 in float, the rest in double */
PCX_API double pcx_trigger_position(const pcx_trigger_hit *hit, double level);
/* rows [starts[e], starts[e] + W) of each of nports buffers (elem_bytes[p] bytes per element, any byte address) into outs[p], an
 * nev x W matrix of the same elements; one launch for all ports, at most PCX_TRIGGER_MAX_PORTS of them.  Every row must lie inside
 * its buffer: nothing can check that.  capture takes host arrays; a buffer may be pageable (the span of the rows is staged),
 * page-locked or device memory.  capture_dev takes device pointers throughout (ins_dev, outs_dev: host arrays of device pointers;
 * starts_dev: a device array), allocates nothing and synchronises nothing. */
PCX_API int pcx_trigger_capture(pcx_trigger *h, size_t nports, const void *const *ins, const size_t *elem_bytes, const uint64_t *starts, size_t nev, size_t W,
                                void *const *outs);
PCX_API int pcx_trigger_capture_dev(pcx_trigger *h, size_t nports, const void *const *ins_dev, const size_t *elem_bytes, const uint64_t *starts_dev, size_t nev,
                                    size_t W, void *const *outs_dev, void *stream);

/* ===================================================================== *
 *  /comms/preamble_framer      digital/PreambleFramer.cpp
 *  /comms/frame_insert         digital/FrameInsert.cpp, digital/FrameHelper.hpp
 *
 *  A stream with a preamble in front of every start label and zero padding behind every end label.  The framer works on bytes; the
 *  inserter on complex symbols, where every preamble symbol is repeated symbol_width times and 58 BPSK header symbols follow: the
 *  Hamming(8,4)-coded id, twelve bits of the length and a checksum over id and all sixteen bits of the length.  The host walks the
 *  call's labels as the reference's loop does and one kernel writes the framed stream as ONE buffer.  Every output
 *  element is a copy, a zero or a sign flip: exact.
 * ===================================================================== */
typedef struct pcx_framer pcx_framer;
enum { PCX_FRAME_OTHER = 0, PCX_FRAME_START = 1, PCX_FRAME_END = 2 };                       /* pcx_frame_event.kind */
enum { PCX_SEG_INPUT = 0, PCX_SEG_POOL = 1, PCX_SEG_HEADER = 2, PCX_SEG_ZERO = 3 };         /* pcx_frame_segment.kind */
#define PCX_FRAME_HEADER_BITS 58
/* a label of the call, in the order of the port (ascending index).  kind: START when its id is the start id, else END when it is the
 * end id, else OTHER.  length: the header's length field, already reduced modulo 65536 (FrameInsert.cpp:231-234: data * width when
 * the data converts to size_t, else 0); ignored without a header */
typedef struct pcx_frame_event {
    uint64_t index, width;
    uint32_t kind, length;
} pcx_frame_event;
/* one run of the output, in elements; it ends where the next entry begins.  src: INPUT the input element, POOL the element of the
 * sync word (the preamble with every symbol repeated), HEADER the index of the frame's word of header bits, ZERO nothing */
typedef struct pcx_frame_segment {
    uint64_t dst, src;
    uint32_t kind, reserved;
} pcx_frame_segment;
typedef struct pcx_frame_plan {
    uint64_t consumed;        /* input elements the call consumes */
    uint64_t used_events;     /* events the call handled: each is consumed with the input */
    uint64_t out_len;         /* output elements */
    uint64_t n_segments;      /* entries of the table, the sentinel {out_len, 0, ZERO} included */
    uint64_t n_headers;       /* words of header bits: one per start event when a header follows */
    int cut;                  /* the capacity ended the call in front of an event */
} pcx_frame_plan;
/* (scalar, is_complex) in {(PCX_U8, 0), (PCX_F32, 1), (PCX_F64, 1)}, anything else is PCX_ERR_ARG "unsupported type".  Preamble {1},
 * symbol width 1, no header, header id 0x55, padding 0. */
PCX_API int pcx_framer_create(pcx_framer **out, int scalar, int is_complex);
PCX_API int pcx_framer_destroy(pcx_framer *h);
/* count elements of the handle's type; an empty preamble and a symbol width of 0 are PCX_ERR_ARG (PreambleFramer.cpp:96,
 * FrameInsert.cpp:120, :142), as is a header on a byte stream.  The sync word is uploaded where a device can be reached, else at
 * the first call that computes. */
PCX_API int pcx_framer_set_preamble(pcx_framer *h, const void *symbols, size_t count, size_t symbol_width, int with_header);
PCX_API int pcx_framer_get_preamble(const pcx_framer *h, void *symbols, size_t cap, size_t *count, size_t *symbol_width, int *with_header);
PCX_API int pcx_framer_set_header_id(pcx_framer *h, unsigned char id);
PCX_API int pcx_framer_get_header_id(const pcx_framer *h, unsigned char *id);
PCX_API int pcx_framer_set_padding(pcx_framer *h, size_t elements);
PCX_API int pcx_framer_get_padding(const pcx_framer *h, size_t *elements);
/* output BYTES a workgroup writes (a multiple of 16: the seams a test wants to straddle) and the longest slice of the segment table
 * a workgroup keeps on chip */
PCX_API int pcx_framer_get_geometry(size_t *tile_bytes, size_t *lds_segments);
/* time sync 0, 1, then the seven Hamming(8,4) words: bit i of *bits is the i-th header symbol's bit.  Twelve bits of the length are
 * coded, the checksum covers all sixteen (FrameHelper.hpp). */
PCX_API int pcx_frame_header_bits(unsigned id, unsigned length, uint64_t *bits);
/* HOST ONLY, no device is touched: what a call on n_in input elements with room for out_cap output elements does.  used, insert_at
 * and shift (each NULL or n_events long) receive per event: whether the call handles it; where its insert begins in the output (an
 * OTHER event: where its label lands); what the block adds to the label's index.  segs / header_words receive the first seg_cap /
 * hdr_cap entries.  The walk is the reference's, with two differences: an event whose head would end in front of what
 * is already passed on has an empty head; and the output is bounded -- events are taken in groups (an event and those behind it at
 * the same index or in front of what the group passed on), a group whole and with the element its last label sits on, the call ends
 * in front of the first group that does not fit (or at the capacity), and a group that exceeds an empty output buffer is PCX_ERR_ARG
 * with both sizes in the message. */
PCX_API int pcx_framer_plan(const pcx_framer *h, size_t n_in, size_t out_cap, const pcx_frame_event *events, size_t n_events, pcx_frame_plan *plan,
                            unsigned char *used, uint64_t *insert_at, uint64_t *shift, pcx_frame_segment *segs, size_t seg_cap,
                            uint64_t *header_words, size_t hdr_cap);
/* plans and runs: out receives plan->out_len elements.  in and the out_cap elements of out must not share a byte (PCX_ERR_ARG
 * "overlaps").  The events are host memory in both forms.  process takes host pointers (staged, or in place when page-locked);
 * process_dev takes device pointers and enqueues on `stream`: the table is uploaded from host memory behind the stream, and the
 * HOST waits for the call before the previous one where it reuses that call's table slot.  Unlike the calls of the other handles it
 * can therefore NOT be captured into a graph: a captured stream has no host plan to run again and no event to wait for. */
PCX_API int pcx_framer_process(pcx_framer *h, const void *in, size_t n_in, const pcx_frame_event *events, size_t n_events, void *out, size_t out_cap,
                               pcx_frame_plan *plan, unsigned char *used, uint64_t *insert_at, uint64_t *shift);
PCX_API int pcx_framer_process_dev(pcx_framer *h, const void *in_dev, size_t n_in, const pcx_frame_event *events, size_t n_events, void *out_dev,
                                   size_t out_cap, pcx_frame_plan *plan, unsigned char *used, uint64_t *insert_at, uint64_t *shift, void *stream);

/* ===================================================================== *
 *  /comms/frame_sync           digital/FrameSync.cpp, digital/FrameHelper.hpp
 *
 *  The receiver of /comms/frame_insert's frame: it searches the stream for the sync word (every preamble symbol held symbol_width *
 *  data_width samples), estimates scale, frequency offset and phase there, reads the 58 BPSK header symbols behind it and passes the
 *  payload on: as it is but scaled (RAW), turned back by the estimated carrier (PHASE), also resampled to one element per data symbol
 *  (TIMING), or from the sync word on (DEBUG).  One call is one work() of the reference; the state it carries from call to call lives in
 *  the handle and activate() resets it.  DESIGN.md 24 has the method and the places where the port differs (symbol widths below 3; a
 *  sync word of at most 65536 samples).  The handle keeps no history of the stream: a frame may begin in front of the buffer of the call
 *  that declares it, but neither the reference nor this port reads anything there.  All device arithmetic is double for both element types.
 * ===================================================================== */
typedef struct pcx_fsync pcx_fsync;
enum { PCX_FSYNC_RAW = 0, PCX_FSYNC_PHASE = 1, PCX_FSYNC_TIMING = 2, PCX_FSYNC_DEBUG = 3 };            /* the output mode */
enum { PCX_FSYNC_PHASE_OFFSET = 0, PCX_FSYNC_FRAME_START = 1, PCX_FSYNC_FRAME_END = 2 };               /* pcx_fsync_label.kind, label ids */
/* a label the call posts on its output: index and width in output elements from the call's first.  value: the phase in radians
 * (PHASE_OFFSET); length: the header's length field (all three kinds) */
typedef struct pcx_fsync_label {
    uint32_t kind, reserved;
    uint64_t index, width, length;
    double value;
} pcx_fsync_label;
typedef struct pcx_fsync_result {
    uint64_t consumed, produced;      /* input elements consumed, output elements written */
    uint64_t reserve;                 /* the input port's reserve after the call (it stays until a later call changes it) */
    uint32_t n_labels, reserved;
    pcx_fsync_label labels[3];        /* in the order they are posted: phase offset, frame start, frame end */
    /* the state after the call */
    uint64_t remaining;               /* payload elements still to come (input elements); 0: searching */
    double phase, phase_inc;          /* the carrier phase at the next payload element, and its step per input element */
    double scale, delta_fc, phase_off;/* the estimates at the last correlation maximum */
    uint64_t max_peak, count_since_max;
} pcx_fsync_result;
/* (scalar, is_complex) in {(PCX_F32, 1), (PCX_F64, 1)}, anything else is PCX_ERR_ARG "unsupported type".  The constructor's settings
 * (:185-193): mode RAW, preamble {1}, header id 0x55, symbol width 20, data width 4, input threshold 0.01, frame start id "frameStart",
 * the other two ids empty. */
PCX_API int pcx_fsync_create(pcx_fsync **out, int scalar, int is_complex);
PCX_API int pcx_fsync_destroy(pcx_fsync *h);
/* an unknown mode, an empty preamble, a data width below 2 and a negative threshold are PCX_ERR_ARG as they are exceptions in the
 * reference (:202, :217, :251, :293).  A symbol width below 3 is PCX_ERR_ARG too: the reference takes 1 and 2 and then averages over
 * an empty or wrapped window.  A sync word (symbol width * data width * preamble symbols) beyond 65536 samples is
 * PCX_ERR_ARG as well, which the reference does not know: one lane walks the word once per candidate frame.  The threshold is kept in
 * the stream's precision.  A setter touches no device; where a width or the preamble changed, the next call waits for the handle's
 * enqueued calls and uploads the preamble. */
PCX_API int pcx_fsync_set_output_mode(pcx_fsync *h, int mode);
PCX_API int pcx_fsync_get_output_mode(const pcx_fsync *h, int *mode);
PCX_API int pcx_fsync_set_preamble(pcx_fsync *h, const void *symbols, size_t count);
PCX_API int pcx_fsync_get_preamble(const pcx_fsync *h, void *symbols, size_t cap, size_t *count);
PCX_API int pcx_fsync_set_header_id(pcx_fsync *h, unsigned char id);
PCX_API int pcx_fsync_get_header_id(const pcx_fsync *h, unsigned char *id);
PCX_API int pcx_fsync_set_symbol_width(pcx_fsync *h, size_t width);
PCX_API int pcx_fsync_get_symbol_width(const pcx_fsync *h, size_t *width);
PCX_API int pcx_fsync_set_data_width(pcx_fsync *h, size_t width);
PCX_API int pcx_fsync_get_data_width(const pcx_fsync *h, size_t *width);
PCX_API int pcx_fsync_set_input_threshold(pcx_fsync *h, double threshold);
PCX_API int pcx_fsync_get_input_threshold(const pcx_fsync *h, double *threshold);
/* accepted and kept; nothing is printed */
PCX_API int pcx_fsync_set_verbose(pcx_fsync *h, int enable);
/* the id of the labels of `kind`; an empty id (or NULL) means that the label is not posted.  get copies at most cap bytes, the
 * terminator included, and sets *len to the id's length */
PCX_API int pcx_fsync_set_label_id(pcx_fsync *h, int kind, const char *id);
PCX_API int pcx_fsync_get_label_id(const pcx_fsync *h, int kind, char *id, size_t cap, size_t *len);
/* the derived settings (updateSettings, :342-348): the sync word and the frame head in samples, the two correlation thresholds; the
 * offsets a workgroup of the search kernel owns; and the offsets of the first piece of a search call -- a call correlates its offsets in
 * pieces, each twice as long as the one before, and stops behind the piece in which a frame is found (the seams a test wants to
 * straddle) */
PCX_API int pcx_fsync_get_geometry(const pcx_fsync *h, size_t *sync_width, size_t *frame_width, size_t *corr_mag, size_t *corr_dur, size_t *tile,
                                   size_t *first_piece);
/* activate() (:326-333): back to searching, phase and tracker cleared; the reported estimates and the reserve are cleared too (the
 * reference leaves those members as they are; it reads none of them before it has set them) */
PCX_API int pcx_fsync_activate(pcx_fsync *h);
/* one work() on n_in input elements with room for out_cap output elements.  While a payload remains the call only enqueues: nothing
 * is read back and process_dev does not synchronise.  A SEARCH call reads a few words back per candidate frame and therefore waits
 * for the stream before it returns.  No form can be captured into a graph: the handle's state advances on the host.  in and out must
 * not share a byte.  process takes host pointers (staged, or in place when page-locked); process_dev device pointers, at any 8-byte
 * (complex_float32) or 16-byte (complex_float64) aligned address.  Checked in this order before any device call: the handle, the
 * result, in, out. */
PCX_API int pcx_fsync_process(pcx_fsync *h, const void *in, size_t n_in, void *out, size_t out_cap, pcx_fsync_result *result);
PCX_API int pcx_fsync_process_dev(pcx_fsync *h, const void *in_dev, size_t n_in, void *out_dev, size_t out_cap, pcx_fsync_result *result, void *stream);

/* ===================================================================== *
 *  /comms/symbol_mapper      digital/SymbolMapper.cpp
 *
 *  out[i] = map[in[i] & mask] (:89-91): one unsigned char in, one element of the stream type out.  Exact.
 * ===================================================================== */
typedef struct pcx_mapper pcx_mapper;
/* SymbolMapperFactory(dtype), :106-122: scalar in {F64, F32, I64, I32, I16, I8}, real or complex; anything else is PCX_ERR_ARG
 * "unsupported type".  The constructor's map is {1} (:58). */
PCX_API int pcx_mapper_create(int scalar, int is_complex, pcx_mapper **out);
PCX_API int pcx_mapper_destroy(pcx_mapper *h);
/* setMap (:66-77): n elements in the stream type's own layout (an int64 map is exact; complex is re, im interleaved).  Checked in this
 * order: the handle, n == 0 "Map must be nonzero size", n not a power of two "Map must be a power of two in length", a null map.
 * mask = (unsigned char)((1 << log2(n)) - 1): a map of 512 entries has mask 255 and uses its first 256, a map of 1 entry mask 0. */
PCX_API int pcx_mapper_set_map(pcx_mapper *h, const void *map, size_t n);
/* *n = the map's length; the first min(*n, cap) elements go to out (out may be NULL when cap is 0) */
PCX_API int pcx_mapper_get_map(const pcx_mapper *h, void *out, size_t cap, size_t *n);
/* work()'s loop (:79-95) over n elements.  Checked in this order before any device call: the handle, n == 0 (nothing to do), null
 * buffers, any overlap of the n input bytes with the output.  process_dev synchronises nothing and allocates nothing: it can be
 * captured into a graph.  The reference counts the elements of a call in 32 bits; n here is a size_t and is not truncated. */
PCX_API int pcx_mapper_process(pcx_mapper *h, const void *in, void *out, size_t n);
PCX_API int pcx_mapper_process_dev(pcx_mapper *h, const void *in_dev, void *out_dev, size_t n, void *stream);

/* ===================================================================== *
 *  /comms/symbol_slicer      digital/SymbolSlicer.cpp
 *
 *  out[i] = the index, stored into an unsigned char, of the first map entry whose float distance to in[i] is strictly smallest,
 *  starting from (0, FLT_MAX) (:88-97).  Real types: (float)abs(map[j] - in[i]) in the promoted element type (:43-46); complex types:
 *  the two differences converted to float, two rounded products and one rounded sum (:49-52).  Exact; int32 / int64 differences that
 *  leave the signed type wrap, where the reference is undefined.
 * ===================================================================== */
typedef struct pcx_slicer pcx_slicer;
/* SymbolSlicerFactory(dtype), :111-127: the mapper's type matrix.  The constructor's map is {1} (:64). */
PCX_API int pcx_slicer_create(int scalar, int is_complex, pcx_slicer **out);
PCX_API int pcx_slicer_destroy(pcx_slicer *h);
/* setMap (:72-76): n elements in the stream type's own layout, any n but 0 ("Map must be nonzero size"; then a null map; the handle
 * first) */
PCX_API int pcx_slicer_set_map(pcx_slicer *h, const void *map, size_t n);
PCX_API int pcx_slicer_get_map(const pcx_slicer *h, void *out, size_t cap, size_t *n);
/* samples a lane and a workgroup hold, the longest map of the on-chip plan (longer ones are read from global memory) and the elements
 * of a call slice: the seams a test wants to straddle */
PCX_API int pcx_slicer_get_geometry(const pcx_slicer *h, size_t *lane, size_t *group, size_t *max_onchip_map, size_t *slice);
/* work()'s loop (:78-101) over n elements; checks and graph capture as pcx_mapper_process (the overlap is that of the input elements
 * with the n output bytes) */
PCX_API int pcx_slicer_process(pcx_slicer *h, const void *in, void *out, size_t n);
PCX_API int pcx_slicer_process_dev(pcx_slicer *h, const void *in_dev, void *out_dev, size_t n, void *stream);

/* ===================================================================== *
 *  /comms/differential_encoder, /comms/differential_decoder      digital/DifferentialEncoder.cpp, digital/DifferentialDecoder.cpp
 *
 *  One unsigned char per symbol in and out, a uint32_t symbols (2 at first) and a carried byte (0 at first) that survives calls and
 *  set_symbols.  Encoder (:59-63): last = (uint8_t)((in[i] + last + symbols) % symbols) in uint32_t, out[i] = last.  Decoder (:59-64):
 *  out[i] = (uint8_t)((in[i] - in[i-1] + symbols) % symbols) in uint32_t, in[-1] the carried byte.  Exact.
 * ===================================================================== */
typedef struct pcx_diffcode pcx_diffcode;
/* pcx_diffcode_get_plan: SCAN when the encoder's step equals (in + last) mod min(symbols, 256) for all 65536 byte pairs (checked in
 * set_symbols), SERIAL (one thread, the reference's loop) otherwise; the decoder always reports SCAN */
enum { PCX_DIFF_SCAN = 0, PCX_DIFF_SERIAL = 1 };
/* decode = 0 the encoder, otherwise the decoder (:30 of either file) */
PCX_API int pcx_diffcode_create(int decode, pcx_diffcode **out);
PCX_API int pcx_diffcode_destroy(pcx_diffcode *h);
/* setSymbols (:37-40).  DEVIATION: symbols == 0 (a division by zero in the reference) is PCX_ERR_ARG "symbols cannot be 0", checked
 * after the handle; the previous value is kept.  The carried byte is left alone. */
PCX_API int pcx_diffcode_set_symbols(pcx_diffcode *h, uint32_t symbols);
PCX_API int pcx_diffcode_get_symbols(const pcx_diffcode *h, uint32_t *symbols);
PCX_API int pcx_diffcode_get_plan(const pcx_diffcode *h, int *plan);
/* bytes a workgroup and a call slice hold (the seams a test wants to straddle) */
PCX_API int pcx_diffcode_get_geometry(size_t *tile, size_t *slice);
/* the carried byte after the handle's last call (waits for it) */
PCX_API int pcx_diffcode_get_state(pcx_diffcode *h, unsigned char *last);
/* the carried byte back to 0 (for API users: the blocks never call it, as the reference has no activate()) */
PCX_API int pcx_diffcode_reset(pcx_diffcode *h);
/* work()'s loop over n bytes, the byte carried across calls.  out may be in itself (in place); any other overlap is PCX_ERR_ARG.
 * Checked in this order before any device call: the handle, n == 0, null buffers, the overlap.  process_dev synchronises nothing and
 * allocates nothing: it can be captured into a graph.  n is a size_t and is not truncated to 32 bits as the reference's count is. */
PCX_API int pcx_diffcode_process(pcx_diffcode *h, const void *in, void *out, size_t n);
PCX_API int pcx_diffcode_process_dev(pcx_diffcode *h, const void *in_dev, void *out_dev, size_t n, void *stream);

/* ===================================================================== *
 *  /comms/bits_to_symbols, /comms/symbols_to_bits, /comms/bytes_to_symbols, /comms/symbols_to_bytes   (digital/)
 *
 *  The four conversions of digital/SymbolHelpers.hpp between bits (one per byte), symbols of `modulus` = 1 ... 8 bits (one per byte)
 *  and payload bytes, in MSBit or LSBit order.  uint8 in, uint8 out, no state between calls.  Every output byte equals the
 *  reference's loop for all 256 values of every input byte:
 *    bits -> symbols   (:13-41)    an input byte counts as 1 when it is not 0
 *    symbols -> bits   (:46-72)    only the low `modulus` bits of a symbol are looked at; outputs are 0 or 1
 *    bytes -> symbols  (:233-414)  outputs are below 2^modulus
 *    symbols -> bytes  (:77-228)   the reference ORs shifted symbols it never masks: the whole 8-bit value of a symbol is placed with
 *                                  its bit 0 on its field's lowest bit and cut off at the upper edge of the last byte the field
 *                                  touches, so bits above the width land on the fields above it
 *  DEVIATION: the packet path of the four blocks (msgWork, e.g. BytesToSymbols.cpp:91-119) has no counterpart here: it rounds a
 *  packet up to whole groups and reads past the payload's end to do so, which is undefined.
 * ===================================================================== */
typedef struct pcx_repack pcx_repack;
enum { PCX_REPACK_BITS_TO_SYMBOLS = 0, PCX_REPACK_SYMBOLS_TO_BITS = 1,
       PCX_REPACK_BYTES_TO_SYMBOLS = 2, PCX_REPACK_SYMBOLS_TO_BYTES = 3 };
/* The constructors' values, not the descriptions' defaults: modulus 1 for all four, MSBit for the two bit kinds
 * (BitsToSymbols.cpp:49, SymbolsToBits.cpp:46), LSBit for the two byte kinds (BytesToSymbols.cpp:43-46, SymbolsToBytes.cpp:46-49).
 * Checked in this order: out, then the kind (unknown: PCX_ERR_ARG). */
PCX_API int pcx_repack_create(int kind, pcx_repack **out);
PCX_API int pcx_repack_destroy(pcx_repack *h);
/* setModulus (:64-71 of BitsToSymbols.cpp, the same in the other three): outside 1 ... 8 is PCX_ERR_ARG
 * "Modulus must be between 1 and 8 inclusive", checked after the handle; the previous value is kept. */
PCX_API int pcx_repack_set_modulus(pcx_repack *h, unsigned mod);
PCX_API int pcx_repack_get_modulus(const pcx_repack *h, unsigned *mod);
/* setBitOrder (:78-83): msb != 0 is "MSBit", 0 is "LSBit" (the blocks map the strings and refuse any other with "Order must be
 * LSBit or MSBit") */
PCX_API int pcx_repack_set_bit_order(pcx_repack *h, int msb);
PCX_API int pcx_repack_get_bit_order(const pcx_repack *h, int *msb);
/* the indivisible unit the reference reserves, in input and output elements: bits -> symbols (w, 1), symbols -> bits (1, w),
 * bytes -> symbols _reserveBytes = 1, 1, 3, 1, 5, 3, 7, 1 at w = 1 ... 8 (BytesToSymbols.cpp:69-76) and the 8 in / w symbols they
 * hold, symbols -> bytes _reserveSyms = 8, 4, 8, 2, 8, 4, 8, 1 (SymbolsToBytes.cpp:72-79) and their in w / 8 bytes */
PCX_API int pcx_repack_get_group(const pcx_repack *h, size_t *in_elems, size_t *out_elems);
/* input elements a workgroup and a call slice hold at the handle's setting (the seams a test wants to straddle) */
PCX_API int pcx_repack_get_geometry(const pcx_repack *h, size_t *tile, size_t *slice);
/* n counts INPUT elements; the output holds n / in_group * out_group elements.  Checked in this order before any device call: the
 * handle, n == 0 (nothing to do: PCX_OK), n not a whole number of groups (PCX_ERR_ARG "not a whole group"), null buffers, any
 * overlap of the input bytes with the output bytes.  process_dev synchronises nothing and allocates nothing: it can be captured
 * into a graph.  n is a size_t and every index in the kernels is 64-bit. */
PCX_API int pcx_repack_process(pcx_repack *h, const void *in, void *out, size_t n);
PCX_API int pcx_repack_process_dev(pcx_repack *h, const void *in_dev, void *out_dev, size_t n, void *stream);

/* ===================================================================== *
 *  /comms/waveform_source, /comms/noise_source   (waveform/)
 *
 *  The two blocks that produce a stream.  Both walk a table of the output type cyclically from a carried index
 *  (WaveformSource.cpp:98-108, NoiseSource.cpp:109-117): out[i] = table[(index + i * step) & (entries - 1)], the arithmetic modulo
 *  2^64 as the reference's size_t is (a negative frequency is a huge step).  Every output is a table entry, so it is the reference's
 *  bit for bit.  pcx_source is that walk on the device; the tables are built on the host by pcx_waveform_table and pcx_noise_table,
 *  which restate updateTable() of the two blocks and need no device.
 * ===================================================================== */
typedef struct pcx_source pcx_source;
/* A source of elements of (scalar, is_complex): any of the twelve stream types, an element of 1 to 16 bytes.  No table yet: generate
 * is PCX_ERR_STATE until set_table.  The carried index starts at 0. */
PCX_API int pcx_source_create(int scalar, int is_complex, pcx_source **out);
PCX_API int pcx_source_destroy(pcx_source *h);
/* The table (`entries` elements in the stream type's layout, copied) and the step of the walk.  entries must be a power of two of at
 * most 2^20 (PCX_ERR_ARG "table size must be a power of two of at most 1048576 entries"), checked after the handle and before the
 * table pointer.  The carried index is kept: it enters the new table as _index does after setFrequency. */
PCX_API int pcx_source_set_table(pcx_source *h, const void *table, size_t entries, uint64_t step);
PCX_API int pcx_source_get_index(const pcx_source *h, uint64_t *index);
PCX_API int pcx_source_set_index(pcx_source *h, uint64_t index);
/* tile: the elements one workgroup writes per pass (16 KiB of output); period: entries / gcd(step mod entries, entries), after how
 * many elements the stream repeats (0 while there is no table); staged: whether that period is held in LDS (else read from global
 * memory) */
PCX_API int pcx_source_get_geometry(const pcx_source *h, size_t *tile, size_t *period, int *staged);
/* The next n elements.  Checked in this order: the handle, n == 0 (nothing to do: PCX_OK, the index stays), the buffer, the table.
 * generate writes host, page-locked or device memory and returns with the elements in `out`.  generate_dev only enqueues: it
 * synchronises nothing and allocates nothing once a table is set, so it can be captured into a graph.  THE CARRIED INDEX IS HOST
 * STATE: it advances by n * step when the call is MADE, not when it runs, so a captured call replays the window it was captured
 * with, every time, and the index moves on by one window per capture and by none per replay.  That holds while the handle's
 * settings stand: the graph reads the handle's device copy of one period of the walk, which the first generate call after a
 * set_table, or after a set_index on a walk whose step is not 1, writes again in place (replays then emit windows of the NEW
 * period), and which a set_table with a longer period reallocates (the graph then reads freed memory: capture again after any
 * set_table).  n is a size_t, every index in the kernels is 64-bit, `out` may have any alignment the element type allows. */
PCX_API int pcx_source_generate(pcx_source *h, void *out, size_t n);
PCX_API int pcx_source_generate_dev(pcx_source *h, void *out_dev, size_t n, void *stream);

/* updateTable() and setElem() of the waveform source (WaveformSource.cpp:178-259) on the host, in double and in the reference's
 * order: the table size doubles from 4096 up to 2^20 while |llround(frac * size)| < 16, frac = (res == 0 ? freq : res) / rate;
 * *step = size_t(llround(freq / rate * size)); entry i is Type(ampl * wave(i) + offset), real types taking the real part and
 * integers converting by C++ truncation; wave is PCX_WAVE_CONST 1, PCX_WAVE_SINE std::polar(1.0, 2 pi i / size), PCX_WAVE_RAMP and
 * PCX_WAVE_SQUARE with the quadrature component at (i + 3 size / 4) % size.
 * table == NULL or cap == 0 only computes *entries and *step; else cap (elements) below *entries is PCX_ERR_ARG.
 * An unknown wave is PCX_ERR_ARG "unknown waveform setting", a step of 0 at freq != 0 PCX_ERR_ARG "step size not achievable". */
enum { PCX_WAVE_CONST = 0, PCX_WAVE_SINE = 1, PCX_WAVE_RAMP = 2, PCX_WAVE_SQUARE = 3 };
PCX_API int pcx_waveform_table(int scalar, int is_complex, int wave, double rate, double freq, double res, double ampl_re, double ampl_im,
                               double offset_re, double offset_im, void *table, size_t cap, size_t *entries, uint64_t *step);

/* The generator of the noise source: a std::mt19937 and the four distributions as NoiseSource.cpp:188-250 calls them, on the host.
 * use_seed == 0 seeds from std::random_device as the reference's constructor does; else from `seed`.
 * pcx_noise_table fills the PCX_NOISE_ENTRIES entries Type(ampl * complex(a, b) + offset), b drawn BEFORE a (the reference leaves the
 * order to its compiler; built with g++ it draws the imaginary component first: tests/golden/make_source_golden.py records it): PCX_NOISE_UNIFORM over [mean - b, mean + b), PCX_NOISE_NORMAL
 * (mean, b), PCX_NOISE_LAPLACE from the uniform distribution AS IT WAS LAST SET (the reference's LAPLACE branch sets it to
 * [mean - b, mean + b) and takes mean -+ b log(1 -+ u)), PCX_NOISE_POISSON (mean).  An unknown wave is PCX_ERR_ARG
 * "unknown waveform setting".  pcx_noise_next_offset is the draw of every work(): uniform_int_distribution<size_t>(0, 4095). */
typedef struct pcx_noise pcx_noise;
enum { PCX_NOISE_UNIFORM = 0, PCX_NOISE_NORMAL = 1, PCX_NOISE_LAPLACE = 2, PCX_NOISE_POISSON = 3 };
#define PCX_NOISE_ENTRIES 4096
PCX_API int pcx_noise_create(int use_seed, uint32_t seed, pcx_noise **out);
PCX_API int pcx_noise_destroy(pcx_noise *h);
PCX_API int pcx_noise_table(pcx_noise *h, int scalar, int is_complex, int wave, double mean, double b, double ampl_re, double ampl_im,
                            double offset_re, double offset_im, void *table);
PCX_API int pcx_noise_next_offset(pcx_noise *h, size_t *draw);

/* ===================================================================== *
 *  /comms/rotate, /comms/scale, /comms/abs, /comms/conjugate   (math/)
 *  Stateless maps; n counts stream elements times dtype.dimension().
 * ===================================================================== */
/* arrayRotate, Rotate.cpp:15-23.  (phasor_re, phasor_im) is std::polar(1.0, phase)
 * BEFORE floatToQ (Rotate.cpp:74); pass (0,0) for a block whose setPhase was never
 * called (value-initialised _phasor).  Complex element types only (:143-157). */
PCX_API int pcx_rotate(int scalar, double phasor_re, double phasor_im, const void *in, void *out, size_t n);
PCX_API int pcx_rotate_dev(int scalar, double phasor_re, double phasor_im, const void *in_dev, void *out_dev, size_t n, void *stream);
/* arrayScale, Scale.cpp:15-23 with factorScaled = floatToQ(factor) (:70-74); real factor */
PCX_API int pcx_scale(int scalar, int is_complex, double factor, const void *in, void *out, size_t n);
PCX_API int pcx_scale_dev(int scalar, int is_complex, double factor, const void *in_dev, void *out_dev, size_t n, void *stream);
/* the same two maps under an explicit Q-format reading (integer element types; q == NULL: the process-wide one) */
PCX_API int pcx_rotate_q(int scalar, double phasor_re, double phasor_im, const pcx_qformat *q, const void *in, void *out, size_t n);
PCX_API int pcx_rotate_q_dev(int scalar, double phasor_re, double phasor_im, const pcx_qformat *q, const void *in_dev, void *out_dev, size_t n,
                             void *stream);
PCX_API int pcx_scale_q(int scalar, int is_complex, double factor, const pcx_qformat *q, const void *in, void *out, size_t n);
PCX_API int pcx_scale_q_dev(int scalar, int is_complex, double factor, const pcx_qformat *q, const void *in_dev, void *out_dev, size_t n,
                            void *stream);
/* Abs.cpp:40-43 via getAbs, FxptHelpers.hpp:36-49; out is the real scalar type */
PCX_API int pcx_abs(int scalar, int is_complex, const void *in, void *out, size_t n);
PCX_API int pcx_abs_dev(int scalar, int is_complex, const void *in_dev, void *out_dev, size_t n, void *stream);
/* Conjugate.cpp:36-39; complex element types only */
PCX_API int pcx_conj(int scalar, const void *in, void *out, size_t n);
PCX_API int pcx_conj_dev(int scalar, const void *in_dev, void *out_dev, size_t n, void *stream);

/* /comms/angle (SURVEY 8f "next"): math/Angle.cpp:23-26 via getAngle, FxptHelpers.hpp:14-29;
 * complex element types only, out is the real scalar type */
PCX_API int pcx_angle(int scalar, const void *in, void *out, size_t n);
PCX_API int pcx_angle_dev(int scalar, const void *in_dev, void *out_dev, size_t n, void *stream);

/* /comms/arithmetic (SURVEY 8f "next"): math/Arithmetic.cpp:70-110, out[i] = in0[i] OP in1[i] with the
 * C++ operator of the element type (real or std::complex of f64, f32, (u)int8..64).  The block's
 * work() (:205-231) left-folds its N input ports: call once per extra port with in0 = out.  `out`
 * may be exactly in0 or in1 (the reference forwards input 0's buffer, :157-158).  Integer x / 0
 * traps in the reference; here it yields 0.  Unknown op or type: PCX_ERR_ARG ("unsupported args", :297). */
typedef enum pcx_arith_op { PCX_ARITH_ADD = 0, PCX_ARITH_SUB = 1, PCX_ARITH_MUL = 2, PCX_ARITH_DIV = 3 } pcx_arith_op;
PCX_API int pcx_arith(int scalar, int is_complex, int op, const void *in0, const void *in1, void *out, size_t n);
PCX_API int pcx_arith_dev(int scalar, int is_complex, int op, const void *in0_dev, const void *in1_dev, void *out_dev, size_t n, void *stream);
/* ---- comparators, bitwise maps, byte order, arithmetic with a constant (logic.hip) ----
 * Stateless, exact, one streaming pass each; every buffer may start at any element-aligned byte address.  A constant is passed as ONE
 * element of the stream's type (two scalars for a complex stream).  Aliasing: `out` of a same-width map may be EXACTLY one of its
 * inputs; a comparator's `out` may be its input only for the 1-byte types; any other overlap of the byte ranges is PCX_ERR_ARG and
 * nothing is queued.  n == 0 returns PCX_OK without a launch.  Unknown op, type or width: PCX_ERR_ARG with a message.
 *
 * /comms/comparator, /comms/const_comparator (math/Comparator.cpp, math/ConstComparator.cpp): out[i] = (a[i] OP b[i]) ? 1 : 0 resp.
 * (a[i] OP k) ? 1 : 0, one byte per scalar, the C++ operator of the type (all ten pcx_scalar codes): every ordered comparison and ==
 * with a NaN gives 0, != gives 1, -0.0 == 0.0 gives 1. */
typedef enum pcx_cmp_op { PCX_CMP_GT = 0, PCX_CMP_LT = 1, PCX_CMP_GE = 2, PCX_CMP_LE = 3, PCX_CMP_EQ = 4, PCX_CMP_NE = 5 } pcx_cmp_op;
PCX_API int pcx_compare(int scalar, int op, const void *in0, const void *in1, void *out_u8, size_t n);
PCX_API int pcx_compare_dev(int scalar, int op, const void *in0_dev, const void *in1_dev, void *out_u8_dev, size_t n, void *stream);
PCX_API int pcx_compare_const(int scalar, int op, const void *in, const void *k, void *out_u8, size_t n);
PCX_API int pcx_compare_const_dev(int scalar, int op, const void *in_dev, const void *k, void *out_u8_dev, size_t n, void *stream);
/* /comms/bitwise_unary, /comms/bitwise_binary, /comms/const_bitwise_binary, /comms/bitshift (digital/Bitwise.cpp); the eight integer
 * codes.  pcx_bitwise: NOT takes nin == 1; AND, OR, XOR fold nin >= 2 inputs in ONE pass of nin reads and one write (beyond eight
 * inputs: further passes of `out` and up to seven more).  `out` may be ONE of the inputs, not two of them.  pcx_bitshift: << keeps the low bits, >> is arithmetic for the signed and
 * logical for the unsigned types, as C++'s on the promoted value; a shift at or above the bit width is PCX_ERR_ARG. */
typedef enum pcx_bit_op { PCX_BIT_NOT = 0, PCX_BIT_AND = 1, PCX_BIT_OR = 2, PCX_BIT_XOR = 3 } pcx_bit_op;
PCX_API int pcx_bitwise(int scalar, int op, const void *const *ins, size_t nin, void *out, size_t n);
PCX_API int pcx_bitwise_dev(int scalar, int op, const void *const *ins_dev, size_t nin, void *out_dev, size_t n, void *stream);
PCX_API int pcx_bitwise_const(int scalar, int op, const void *in, const void *k, void *out, size_t n);
PCX_API int pcx_bitwise_const_dev(int scalar, int op, const void *in_dev, const void *k, void *out_dev, size_t n, void *stream);
PCX_API int pcx_bitshift(int scalar, int left, const void *in, size_t shift, void *out, size_t n);
PCX_API int pcx_bitshift_dev(int scalar, int left, const void *in_dev, size_t shift, void *out_dev, size_t n, void *stream);
/* /comms/byte_order (digital/ByteOrder.cpp, ByteOrder.hpp:109-114): each of the n_scalars scalars of `width` = 2, 4 or 8 bytes
 * reversed; a complex element is two scalars */
PCX_API int pcx_byteswap(int width, const void *in, void *out, size_t n_scalars);
PCX_API int pcx_byteswap_dev(int width, const void *in_dev, void *out_dev, size_t n_scalars, void *stream);
/* /comms/const_arithmetic (math/ConstArithmetic.cpp): pcx_arith's operators with the constant as one operand, the twenty element
 * types.  Integer x / 0 yields 0 and MIN / -1 yields MIN, as in pcx_arith. */
typedef enum pcx_arithk_op {
    PCX_ARITHK_X_ADD_K = 0, PCX_ARITHK_X_SUB_K = 1, PCX_ARITHK_K_SUB_X = 2, PCX_ARITHK_X_MUL_K = 3, PCX_ARITHK_X_DIV_K = 4, PCX_ARITHK_K_DIV_X = 5
} pcx_arithk_op;
PCX_API int pcx_arith_const(int scalar, int is_complex, int op, const void *in, const void *k, void *out, size_t n);
PCX_API int pcx_arith_const_dev(int scalar, int is_complex, int op, const void *in_dev, const void *k, void *out_dev, size_t n, void *stream);
/* ---- the real-valued function blocks (mathfn.hip): /comms/exp exp2 exp10 expm1 expN, /comms/log log2 log10 log1p logN, /comms/pow,
 * /comms/sqrt cbrt nth_root, /comms/rsqrt, /comms/sinc, /comms/sigmoid, /comms/trigonometric (math/Exp.cpp, Log.cpp, Pow.cpp, Root.cpp,
 * RSqrt.cpp, Sinc.cpp, Sigmoid.cpp, Trigonometric.cpp; the scalar loops).  PCX_F64 and PCX_F32 only; the reference's integer
 * instantiations are not built and any other type is PCX_ERR_ARG ("unsupported type").
 * Each code is ONE expression of the reference: reciprocal functions 1 / f(x), inverse reciprocal ones f(1 / x), SINC 1 where
 * |x| < 1e-6 and sin(x) / x elsewhere, SIGMOID 1 / (1 + exp(-x)), EXPN pow(base, x), LOGN log(x) / log(base), POW pow(x, exponent),
 * NTH_ROOT pow(x, 1.0 / root) resp. pow(x f, 1.0 / root) f with f = +-1 exactly when fmod(root, 2) == 1.  The choice the reference's
 * setBase / setRoot make between these expressions (base 10 -> EXP10 / LOG10, root 3 -> CBRT, everything else generic, base 2 and
 * root 2 included) is the block's, not this call's.
 * Accuracy: float64 is the device library's function; float32 is the same double expression rounded once (within one unit in the
 * last place of the correctly rounded value).  SQRT, and RSQRT in both types, are exact: RSQRT on float32 is the reference's bit-trick
 * approximation (RSqrt.hpp), not 1 / sqrt.  Where the reference's float32 expression overflows INSIDE (sigmoid(-100), csch(90)) it
 * returns 0 and this returns the small true value.
 * `out` may be exactly `in`; any other overlap is PCX_ERR_ARG.  Buffers may start at any element-aligned byte address.  The codes
 * from PCX_MATH_EXPN on take a parameter -- ONE value of the element type -- and go through pcx_mathfn_param; the others go through
 * pcx_mathfn; either call refuses the other's codes.  A LOGN base <= 0 is PCX_ERR_ARG (Log.cpp:188-191).  Every refusal returns
 * before a device is touched. */
typedef enum pcx_math_fn {
    PCX_MATH_EXP = 0, PCX_MATH_EXP2 = 1, PCX_MATH_EXP10 = 2, PCX_MATH_EXPM1 = 3,
    PCX_MATH_LOG = 4, PCX_MATH_LOG2 = 5, PCX_MATH_LOG10 = 6, PCX_MATH_LOG1P = 7,
    PCX_MATH_SQRT = 8, PCX_MATH_CBRT = 9, PCX_MATH_RSQRT = 10, PCX_MATH_SINC = 11, PCX_MATH_SIGMOID = 12,
    /* /comms/trigonometric, in the order of its description */
    PCX_MATH_COS = 16, PCX_MATH_SIN = 17, PCX_MATH_TAN = 18, PCX_MATH_SEC = 19, PCX_MATH_CSC = 20, PCX_MATH_COT = 21,
    PCX_MATH_ACOS = 22, PCX_MATH_ASIN = 23, PCX_MATH_ATAN = 24, PCX_MATH_ASEC = 25, PCX_MATH_ACSC = 26, PCX_MATH_ACOT = 27,
    PCX_MATH_COSH = 28, PCX_MATH_SINH = 29, PCX_MATH_TANH = 30, PCX_MATH_SECH = 31, PCX_MATH_CSCH = 32, PCX_MATH_COTH = 33,
    PCX_MATH_ACOSH = 34, PCX_MATH_ASINH = 35, PCX_MATH_ATANH = 36, PCX_MATH_ASECH = 37, PCX_MATH_ACSCH = 38, PCX_MATH_ACOTH = 39,
    /* with a parameter: base, base, exponent, root */
    PCX_MATH_EXPN = 48, PCX_MATH_LOGN = 49, PCX_MATH_POW = 50, PCX_MATH_NTH_ROOT = 51
} pcx_math_fn;
PCX_API int pcx_mathfn(int scalar, int fn, const void *in, void *out, size_t n);
PCX_API int pcx_mathfn_dev(int scalar, int fn, const void *in_dev, void *out_dev, size_t n, void *stream);
PCX_API int pcx_mathfn_param(int scalar, int fn, const void *param, const void *in, void *out, size_t n);
PCX_API int pcx_mathfn_param_dev(int scalar, int fn, const void *param, const void *in_dev, void *out_dev, size_t n, void *stream);
/* ---- the special-function blocks (specfn.hip): /comms/gamma, /comms/lngamma, /comms/erf, /comms/erfc, /comms/beta, /comms/modf
 * (math/Gamma.cpp, ErrorFunction.cpp, Beta.cpp, ModF.cpp; the scalar loops).  PCX_F64 and PCX_F32 only; any other type is
 * PCX_ERR_ARG ("unsupported type").  pcx_specfn: std::tgamma, std::lgamma, std::erf, std::erfc of every element.  pcx_beta:
 * exp(lgamma(a) + lgamma(b) - lgamma(a + b)), which is what std::beta computes: a NaN for a NaN, and |B(a, b)| where an argument is
 * negative.  The value is that expression's: from a larger argument of 1024 on, where lgamma(a) and lgamma(a + b) are huge and cancel,
 * their difference is taken from Stirling's series.  pcx_modf: out_frac[i] = std::modf(in[i], &out_int[i]); both parts carry the sign of the input, exactly.
 * Accuracy: as the pcx_mathfn family -- float64 is the device library's function, float32 the same double expression rounded once;
 * special inputs (poles, infinities, signed zeros) give what C prescribes.
 * Aliasing: pcx_specfn's `out` may be exactly `in`; pcx_beta's `out` may be exactly in0 or exactly in1, and the inputs may overlap
 * each other in any way; either output of pcx_modf may be exactly `in`, and the two outputs share no byte.  Any other overlap of an
 * output is PCX_ERR_ARG.  Buffers may start at any element-aligned byte address.  n == 0 is PCX_OK whatever the pointers.  Every
 * refusal returns before a device is touched. */
typedef enum pcx_spec_fn { PCX_SPEC_GAMMA = 0, PCX_SPEC_LNGAMMA = 1, PCX_SPEC_ERF = 2, PCX_SPEC_ERFC = 3 } pcx_spec_fn;
PCX_API int pcx_specfn(int scalar, int fn, const void *in, void *out, size_t n);
PCX_API int pcx_specfn_dev(int scalar, int fn, const void *in_dev, void *out_dev, size_t n, void *stream);
PCX_API int pcx_beta(int scalar, const void *in0, const void *in1, void *out, size_t n);
PCX_API int pcx_beta_dev(int scalar, const void *in0_dev, const void *in1_dev, void *out_dev, size_t n, void *stream);
PCX_API int pcx_modf(int scalar, const void *in, void *out_int, void *out_frac, size_t n);
PCX_API int pcx_modf_dev(int scalar, const void *in_dev, void *out_int_dev, void *out_frac_dev, size_t n, void *stream);
/* /comms/split_complex, /comms/combine_complex: utility/SplitComplex.cpp:10-18, utility/CombineComplex.cpp:10-17;
 * scalar = the real type of the planes (f64, f32, int64..int8: splitComplexFactory :60-70) */
PCX_API int pcx_split_complex(int scalar, const void *in, void *re, void *im, size_t n);
PCX_API int pcx_split_complex_dev(int scalar, const void *in_dev, void *re_dev, void *im_dev, size_t n, void *stream);
PCX_API int pcx_combine_complex(int scalar, const void *re, const void *im, void *out, size_t n);
PCX_API int pcx_combine_complex_dev(int scalar, const void *re_dev, const void *im_dev, void *out_dev, size_t n, void *stream);

/* ===================================================================== *
 *  Fused FM-demod chain  Rotate -> FIR -> FreqDemod in one kernel
 *  (BASELINE.json configs[4]); equals the three blocks above connected in a
 *  topology: Rotate.cpp:15-23 -> FIRFilter.cpp:286-302 (M=L=1) -> FreqDemod.cpp:60-67
 *  complex_float32 in, float32 out.
 * ===================================================================== */
typedef struct pcx_fmchain pcx_fmchain;
PCX_API int pcx_fmchain_create(pcx_fmchain **out);
PCX_API int pcx_fmchain_destroy(pcx_fmchain *h);
PCX_API int pcx_fmchain_set_phase(pcx_fmchain *h, double phase);
/* REAL (complex_taps=0) or COMPLEX taps, as pcx_fir_set_taps */
PCX_API int pcx_fmchain_set_taps(pcx_fmchain *h, const double *taps, size_t ntaps, int complex_taps);
PCX_API int pcx_fmchain_reset(pcx_fmchain *h);
/* PCX_FIR_AUTO (default), PCX_FIR_DIRECT (LDS-tiled time domain) or PCX_FIR_OLS_FFT (K <= 2048) */
PCX_API int pcx_fmchain_set_algo(pcx_fmchain *h, int algo);
PCX_API int pcx_fmchain_last_algo(const pcx_fmchain *h);
PCX_API int pcx_fmchain_set_slots(pcx_fmchain *h, unsigned slots);      /* as pcx_fir_set_slots */
/* in_elems input samples with K-1 history in front -> in_elems-(K-1) demodulated
 * outputs; FreqDemod's prev is carried in the handle */
PCX_API int pcx_fmchain_process(pcx_fmchain *h, const void *in, size_t in_elems, void *out, size_t out_cap,
                                size_t *consumed, size_t *produced);
PCX_API int pcx_fmchain_process_dev(pcx_fmchain *h, const void *in_dev, size_t in_elems, void *out_dev, size_t out_cap,
                                    size_t *consumed, size_t *produced, void *stream);
/* one shard of a sharded chain in ONE launch, as pcx_fir_process_dev_gated: the halo in front of the shard is K samples here
 * (the FIR's K-1 and the one FreqDemod's `_prev` needs, FreqDemod.cpp:63-65); gated for K <= 2048 and long calls */
PCX_API int pcx_fmchain_process_dev_gated(pcx_fmchain *h, const void *in_dev, size_t in_elems, void *out_dev, size_t out_cap,
                                          size_t *consumed, size_t *produced, const void *gate_dev, unsigned gate_value, void *stream,
                                          int *gated);

/* ===================================================================== *
 *  ONE complex_float32 stream over the GPUs of a node  (BASELINE.json configs[3])
 *
 *  The reference has no multi-device story; what makes this possible is in its loop: output n reads inputs
 *  n .. n+K-1 only (FIRFilter.cpp:296-299) and a work() call leaves the last K-1 inputs un-consumed as the next
 *  call's history (:305-307).  A stream of G*C samples is split into G contiguous shards of C samples, one per
 *  device; before every pass shard g receives the LAST K-1 samples of shard g-1 into the slot in front of its own
 *  samples (RCCL ncclSend/ncclRecv, one group per pass, (K-1)*8 bytes per boundary), shard 0 keeps the stream's
 *  own history.  Each shard is ONE kernel launch per pass: everything behind its first block is filtered while the halo is in
 *  flight, the first block last, behind a gate word the halo stream sets (pcx_fir_process_dev_gated).
 *  One process drives all devices (ncclCommInitAll): a Pothos block that owns a pcx_shard spreads its stream over
 *  the node from inside one work() call.  M = L = 1, complex_float32 (the north-star path).
 *
 *  Call order:  create -> set_taps -> configure(C) -> { fill the shard inputs (pcx_shard_buffers gives the device
 *  pointers and the per-device stream to fill them on; or pcx_shard_scatter from one host buffer) -> step }* ->
 *  gather / read the outputs -> destroy.  pcx_shard_step only enqueues; pcx_shard_sync waits.
 * ===================================================================== */
typedef struct pcx_shard pcx_shard;
typedef enum pcx_shard_transport {
    PCX_SHARD_RCCL = 0,      /* ncclSend/ncclRecv over xGMI; one distinct device per shard (RCCL is loaded on first use).  What one GPU could
                              * show about its cost: RCCL's send/recv kernel needs a slot on the device, and beside a gated launch that fills
                              * it (128-VGPR workgroups, RCCL's waves are allocated 136) it gets one only when that launch's first workgroups
                              * exit -- the pass then ends ~18 us late (+9 %; DESIGN.md 6, profiles/r04/rccl_cost_probe.txt).  The rank driver
                              * (pothoscomms_amd/stream.py) hides that by exchanging the NEXT batch's halo; this driver does not. */
    PCX_SHARD_PEER_COPY = 1  /* hipMemcpyPeerAsync between the devices (peer access is switched on where the devices allow it): no kernel
                              * that must find a slot -- two shards on one device cost +1.2 % over one launch.  Several shards may share a
                              * device (how a 1-GPU box rehearses G > 1).  bench.py --driver native --native-transport peer|rccl compares. */
} pcx_shard_transport;
/* devices: `nshards` ordinals, or NULL for 0 .. nshards-1 */
PCX_API int pcx_shard_create(int nshards, const int *devices, int transport, pcx_shard **out);
PCX_API int pcx_shard_destroy(pcx_shard *s);
/* FIRFilter::setTaps on every device's filter, FIRFilter.cpp:138-144; REAL (complex_taps = 0) or COMPLEX taps */
PCX_API int pcx_shard_set_taps(pcx_shard *s, const double *taps, size_t ntaps, int complex_taps);
PCX_API int pcx_shard_set_algo(pcx_shard *s, int algo);                 /* pcx_fir_algo, default PCX_FIR_AUTO */
/* enable != 0: the shards run the fused chain Rotate(phase) -> FIR -> FreqDemod (pcx_fmchain, BASELINE configs[4]) instead of the
 * FIR alone: float32 outputs, a halo of K samples (the FIR's K-1 and FreqDemod's one, FreqDemod.cpp:63-65), every pass from the
 * reset state (the first output of the stream is arg of a zero, FreqDemod.cpp:44-47).  Call before pcx_shard_configure. */
PCX_API int pcx_shard_set_chain(pcx_shard *s, int enable, double phase);
/* allocate, on every device, [halo (K-1) | shard_elems samples] and shard_elems outputs; the halo of shard 0 (the
 * stream's history) starts as zeros, as after FIRFilter::activate */
PCX_API int pcx_shard_configure(pcx_shard *s, size_t shard_elems);
PCX_API int pcx_shard_info(const pcx_shard *s, int *nshards, size_t *K, size_t *shard_elems, int *transport);
/* shard g: in_dev -> K-1 halo samples followed by the shard's own samples; out_dev -> its shard_elems outputs;
 * stream -> the per-device stream (hipStream_t) the pass runs on: fill in_dev on it, or synchronise before a step */
PCX_API int pcx_shard_buffers(pcx_shard *s, int g, void **in_dev, void **out_dev, void **stream, int *device);
/* host_stream: K-1 history samples followed by nshards*shard_elems samples; only shard 0 receives a halo from here */
PCX_API int pcx_shard_scatter(pcx_shard *s, const void *host_stream, size_t elems);
/* one pass over every shard: the halo exchange and ONE launch per shard (pcx_fir_process_dev_gated); configurations without a
 * gated kernel run body, exchange, head as two launches */
PCX_API int pcx_shard_step(pcx_shard *s);
/* pcx_shard_step in its two halves -- the exchange of the halos of what the shard buffers hold NOW (+ the gate signals behind it), and
 * the pass over it -- for DOUBLE-BUFFERED streaming over two handles A and B on the same devices:
 *     fill B (batch k+1);  pcx_shard_compute(A)  [batch k, its exchange posted one turn earlier];  pcx_shard_post_exchange(B);  swap
 * so that the halos of batch k+1 travel while batch k is filtered.  It matters for the RCCL transport, whose send/recv kernel finds a
 * slot beside a gated launch only when that launch's first workgroups exit (PCX_SHARD_RCCL above): a pass that waits for its OWN exchange
 * ends ~18 us late, a pass whose exchange was posted a turn earlier does not (measured for the rank driver, pothoscomms_amd/stream.py
 * PingPongFir: +4 % over the plain launch instead of +9-11 %).  Each handle has its own streams, so the host may queue compute(A) first.
 * After pcx_shard_post_exchange the shard buffers of that handle must not be written until its pcx_shard_compute has been queued (the
 * exchange is reading their tails; compute orders later writers behind it).  compute without a posted exchange, a second post
 * without a compute between, and pcx_shard_scatter / pcx_shard_configure / pcx_shard_set_taps / pcx_shard_set_chain / pcx_shard_set_algo
 * on a handle whose exchange is posted are PCX_ERR_STATE (the setters would change, or free, what the posted pass is about to use). */
PCX_API int pcx_shard_post_exchange(pcx_shard *s);
PCX_API int pcx_shard_compute(pcx_shard *s);
/* enable != 0: one SUBMIT THREAD per DEVICE.  Queueing a pass costs the host 16-20 us per shard from one thread (the cross-stream waits,
 * the records, the gate signal, the launch): 135-165 us for eight shards against a pass of 195 us at 64 Mi samples per shard.  With
 * submit threads every device's share of a pass is queued by a thread of its own, bound to that device (several shards on one device:
 * one thread, in shard order -- threads that call into ONE device's runtime only queue behind its locks); pcx_shard_step /
 * post_exchange / compute still return when everything is queued, and everything the header says about ordering holds unchanged.  The
 * threads spin for ~0.4 ms behind a pass (a stream of passes finds them awake) and sleep after that; they are joined by
 * pcx_shard_destroy or by enable = 0.  Off by default.  PCX_ERR_STATE while an exchange is posted. */
PCX_API int pcx_shard_set_submit_threads(pcx_shard *s, int enable);
/* enable = 0: every shard as TWO launches per pass -- the body while the halo is in flight, the head behind an event on the halo
 * stream -- instead of one gated launch (the default, enable = 1).  The gated launch relies on the halo transfer and its signal,
 * which pcx_shard_step queues BEFORE the launch, reaching the device before it: that is how the runtime submits (in order, from the
 * calling thread) in its default mode.  With AMD_DIRECT_DISPATCH=0 every stream is submitted by a thread of its own and a signal can
 * land behind the launch it is to release, in the same hardware queue: the gate then opens on its two-second bound only and
 * pcx_shard_gather / pcx_shard_sync report PCX_ERR_STATE (measured: intermittently, one test run in three on this stack; never in the
 * default mode, nor with GPU_MAX_HW_QUEUES=1 / 8 or HSA_ENABLE_SDMA=0).  A process that has
 * to run in that mode switches the gate off; the two-launch form costs 5-14 % of a pass. */
PCX_API int pcx_shard_set_gated(pcx_shard *s, int enable);
/* the nshards*shard_elems outputs in stream order (waits for the pass).  PCX_ERR_STATE when a shard's gated launch gave up
 * waiting for its halo during the passes since the last gather / sync (the two-second bound of pcx_fir_process_dev_gated): the
 * outputs are copied all the same, the seam's are wrong, and the condition is cleared by being reported. */
PCX_API int pcx_shard_gather(pcx_shard *s, void *host_out, size_t elems);
/* waits for everything queued on the shards' streams; reports (and clears) a gate timeout like pcx_shard_gather */
PCX_API int pcx_shard_sync(pcx_shard *s);

#ifdef __cplusplus
}
#endif
#endif /* PCX_H */
