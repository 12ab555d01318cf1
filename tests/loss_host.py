"""Host side (no GPU) of the candidate-sweep losses' tests, for "softmax_ce", "sampled_ce" and "gbce": a descriptor that only lacks its
workspace, the refusal of a descriptor, the ctypes mirror against the C layout, and MurmurHash3's finaliser by hand."""
import ctypes
import os
import shutil
import subprocess

import pytest

import castrec_amd  # noqa: F401
from castrec_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DESC = {"softmax_ce": "SoftmaxCeDesc", "sampled_ce": "SampledCeDesc", "gbce": "GbceDesc"}


def valid_desc(loss, M=40, V=100, D=50, N=16):
    """A descriptor that passes every check but the workspace (fake pointers: nothing is launched on a check failure)."""
    d = getattr(L, DESC[loss])()
    d.seq_emb, d.ld, d.table, d.pos, d.neg = 16, D, 16, 16, 16
    d.M, d.D, d.V, d.precision, d.state = M, D, V, L.PREC_BF16X3, 16
    d.d_seq_emb, d.ldd, d.table_grad = 16, D, 16
    if loss != "softmax_ce":
        d.N, d.samples, d.seed, d.step = N, None, 7, 16
    if loss == "gbce":
        d.beta = 0.5
    return d


def rejects(loss, d, *words):
    rc = getattr(L.lib, "cr_" + loss)(ctypes.byref(d) if d is not None else None, None)
    msg = L.lib.cr_last_error().decode()
    assert rc == -1, (rc, msg)
    assert "cr_" + loss in msg
    for w in words:
        assert w in msg, msg
    return msg


def desc_mirror_matches_c_layout(tmp_path, loss, constants=()):
    """sizeof and every offsetof of cr_<loss>_desc, and the named constants of castrec.h, as a C compiler sees them."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    cls = getattr(L, DESC[loss])
    probes = [("sizeof(cr_%s_desc)" % loss, ctypes.sizeof(cls))] + [(c, getattr(L, c)) for c in constants]
    probes += [("offsetof(cr_%s_desc, %s)" % (loss, f), getattr(cls, f).offset) for f, _ in cls._fields_]
    src = tmp_path / "desc.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "castrec.h"\nint main(void){' +
                   "".join('printf("%%zu\\n", (size_t)%s);' % e for e, _ in probes) + 'return 0;}\n')
    exe = tmp_path / "desc"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [n for _, n in probes]


def fmix32_by_hand(h):
    """MurmurHash3's 32-bit finaliser on plain Python integers (cr_common.hpp cr_fmix32)."""
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def hashes_by_hand(seed, step, N, site):
    """The N hashes of a draw at (seed, step, site) on plain Python integers (cr_common.hpp cr_site_key, CR_PHI)."""
    inner = (step * 0x9E3779B9 + site * 0x85EBCA77 + 0x165667B1) & 0xFFFFFFFF
    key = fmix32_by_hand(seed ^ fmix32_by_hand(inner))
    return [fmix32_by_hand((key + j * 0x9E3779B1) & 0xFFFFFFFF) for j in range(N)]


def refuses_the_common_arguments(loss):
    """What every loss's entry refuses before any HIP call: a NULL descriptor or pointer, D, V, M (and N), the pitches, the precision."""
    rejects(loss, None, "NULL descriptor")
    for f in ("seq_emb", "table", "pos", "state"):
        d = valid_desc(loss)
        setattr(d, f, None)
        rejects(loss, d, "NULL")
    for D in (4, 7, 257):
        d = valid_desc(loss); d.D, d.ld, d.ldd = D, 300, 300
        rejects(loss, d, "D=%d" % D)
    for V in (1, 0, -3):
        d = valid_desc(loss); d.V = V
        rejects(loss, d, "V=%d" % V)
    for M in (0, -1):
        d = valid_desc(loss); d.M = M
        rejects(loss, d, "M=%d" % M)
    for N in (0, -2, L.CR_SCE_MAX_SAMPLES + 1) if loss != "softmax_ce" else ():
        d = valid_desc(loss); d.N = N
        rejects(loss, d, "N=%d" % N)
    d = valid_desc(loss); d.ld = 49
    rejects(loss, d, "ld=49")
    d = valid_desc(loss); d.ldd = 10
    rejects(loss, d, "ldd=10")
    d = valid_desc(loss); d.precision = 7
    rejects(loss, d, "precision 7")


def sampled_workspace_query_is_monotone(ws):
    """ws(M, N, D) of a sampled loss: 0 for what the kernel does not take, else growing with M and with N; independent of V, O(M + N D):
    the C5 shape needs well under 100 MB."""
    assert ws(0, 16, 50) == 0 and ws(-1, 16, 50) == 0 and ws(4, 0, 50) == 0 and ws(4, -1, 50) == 0
    assert ws(4, L.CR_SCE_MAX_SAMPLES + 1, 50) == 0 and ws(4, 16, 7) == 0 and ws(4, 16, 257) == 0 and ws(4, 16, 4) == 0
    assert ws(1, 1, 8) > 0 and ws(1, L.CR_SCE_MAX_SAMPLES, 256) > 0
    Ns = (1, 7, 31, 64, 256, 1000, 1024, 1025, 2048, 4096, 10000, 16384)
    Ms = (1, 7, 64, 65, 300, 6400, 25600, 65536, 10 ** 6)
    for D in (8, 20, 50, 64, 128, 256):
        for N in Ns:
            prev = 0
            for M in Ms:
                n = ws(M, N, D)
                assert n > 0 and n >= prev, (D, N, M, n, prev)
                prev = n
        for M in Ms:
            prev = 0
            for N in Ns:
                n = ws(M, N, D)
                assert n > 0 and n >= prev, (D, M, N, n, prev)
                prev = n
    assert ws(128 * 512, 4096, 256) < 100 * 2 ** 20
