"""CPU check of the overlap-save block geometry (csrc/ols_geometry.hpp, plain C++): a host compiler runs the launchers' own function
over a table of cases, and the six values are held against a brute-force statement of which blocks are full.  Once more as a
stand-alone executable under the address and undefined-behaviour sanitizers.  No device is touched."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pothoscomms_amd", "csrc")

DRIVER = r"""
#include "ols_geometry.hpp"
#include <cstdio>
int main(int argc, char **a)
{
    if (argc != 2) return 1;
    FILE *f = std::fopen(a[1], "r");
    if (!f) return 2;
    unsigned long long K, align, N, n_out, in_elems, lead;
    while (std::fscanf(f, "%llu %llu %llu %llu %llu %llu", &K, &align, &N, &n_out, &in_elems, &lead) == 6) {
        const pcx::OlsGeometry g = pcx::ols_geometry(K, align, N, n_out, in_elems, lead);
        std::printf("%zu %zu %zu %zu %zu %zu\n", g.Kov, g.pad, g.S, g.nblocks, g.first_full, g.nfull);
    }
    std::fclose(f);
    return 0;
}
"""


def cases():
    out = []
    for K, align, N in itertools.product((1, 2, 16, 17, 255, 2049), (16, 32), (4096, 8192)):
        Kov = -(-(K - 1) // align) * align
        S, pad = N - Kov, Kov - (K - 1)
        for n_out, short, lead in itertools.product((1, S - 1, S, S + 1, 5 * S + 7), (False, True), (0, pad)):
            need = n_out + K - 1                      # what the call reads for n_out outputs
            out.append((K, align, N, n_out, max(need - S, 0) if short else need, lead))
    return out


def brute_force(K, align, N, n_out, in_elems, lead):
    Kov = next(k for k in range(K - 1, K - 1 + align) if k % align == 0)
    pad, S = Kov - (K - 1), N - Kov
    nblocks = next(nb for nb in range(1, n_out + 2) if nb * S >= n_out)
    full = [b for b in range(nblocks) if -lead <= b * S - pad and b * S - pad + N <= in_elems and b * S + S <= n_out]
    return Kov, pad, S, nblocks, full


def build(tmp_path, name, extra):
    src, exe = tmp_path / "geometry.cpp", tmp_path / name
    src.write_text(DRIVER)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + extra + ["-I" + CSRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def check(exe, tmp_path):
    table = cases()
    assert len(table) == 6 * 2 * 2 * 5 * 2 * 2
    (tmp_path / "cases.txt").write_text("".join("%d %d %d %d %d %d\n" % c for c in table))
    r = subprocess.run([str(exe), str(tmp_path / "cases.txt")], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(table)
    some_full = some_ragged_head = some_cut = 0
    for c, line in zip(table, lines):
        Kov, pad, S, nblocks, first_full, nfull = (int(v) for v in line.split())
        wKov, wpad, wS, wnblocks, full = brute_force(*c)
        assert (Kov, pad, S, nblocks) == (wKov, wpad, wS, wnblocks), c
        if full:
            assert full == list(range(full[0], full[-1] + 1)), c      # one run
            assert (first_full, nfull) == (full[0], full[-1] + 1), (c, full)
        else:
            assert nfull == first_full, c
        assert first_full <= nfull <= nblocks, c
        some_full += bool(full)
        some_ragged_head += bool(full) and full[0] == 1
        some_cut += bool(full) and full[-1] + 1 < c[3] // S
    assert some_full and some_ragged_head and some_cut and some_full < len(table)    # the table reaches every branch of the function


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_geometry_equals_the_brute_force_statement(tmp_path):
    check(build(tmp_path, "geometry", []), tmp_path)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_geometry_runs_clean_under_the_sanitizers(tmp_path):
    """a stand-alone executable: the sanitizer runtimes are linked into it, nothing is preloaded"""
    exe = build(tmp_path, "geometry_san", ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    check(exe, tmp_path)
