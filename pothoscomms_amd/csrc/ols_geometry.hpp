// ols_geometry.hpp -- the block geometry of the overlap-save /comms/fir_filter launchers (fir_ols.hip, fir_ols_decim.hip,
// fir_ols_f64.hip).  Plain C++ on purpose, as repack_core.hpp is: a host compiler runs the same function
// (tests/test_ols_geometry_cpu.py holds it against a brute-force statement of which blocks are full).
//
// A block is N samples long.  Kov >= K-1 outputs are dropped at its head: K-1 rounded up to the alignment, so that every row
// a kernel stores starts on a 128-byte line.  The block's window starts pad = Kov-(K-1) samples before sample b*S, S = N - Kov.
// Block b is FULL -- the kernels' fast load path -- when its window [b*S - pad, b*S - pad + N) lies inside the buffer and all
// S outputs are wanted: the full blocks are first_full <= b < nfull (nfull = first_full: none).
#pragma once
#include <cstddef>

namespace pcx {

struct OlsGeometry {
    size_t Kov, pad, S, nblocks, first_full, nfull;
};

// K taps; align: 16 (8-byte samples), 32 (4-byte samples), 1 keeps the minimal K-1 overlap; n_out: outputs wanted, at the
// block's rate; in_elems: samples readable from the stream's sample 0 on; lead_valid: samples of the same stream readable in
// front of sample 0 (with at least `pad` of them block 0 is a full block like any other).
// An overlap that leaves no output per block (Kov >= N) comes back with S = nblocks = 0: the caller refuses such a K.
inline OlsGeometry ols_geometry(size_t K, size_t align, size_t N, size_t n_out, size_t in_elems, size_t lead_valid)
{
    OlsGeometry g = {};
    const size_t Km1 = K - 1;
    g.Kov = (Km1 + align - 1) / align * align;
    g.pad = g.Kov - Km1;
    if (g.Kov >= N) return g;
    g.S = N - g.Kov;
    g.nblocks = (n_out + g.S - 1) / g.S;
    g.first_full = g.pad > lead_valid ? 1 : 0;
    g.nfull = n_out / g.S;
    while (g.nfull > g.first_full && (g.nfull - 1) * g.S - g.pad + N > in_elems) g.nfull--;
    if (g.nfull < g.first_full) g.nfull = g.first_full;
    return g;
}

}  // namespace pcx
