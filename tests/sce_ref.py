"""numpy restatement of cr_sampled_ce's device draw (castrec.h): key = cr_site_key(seed, step, CR_SCE_SITE), then for each j
x = cr_fmix32(key + j * CR_PHI) and s_j = 1 + ((x * (V - 1)) >> 32)."""
import numpy as np

from dropout_ref import M32, fmix32, site_key

CR_SCE_SITE = 0x5CE00000
CR_PHI = 0x9E3779B1


def draw(seed, step, V, N):
    key = site_key(np.uint64(seed & 0xFFFFFFFF), np.uint64(step & 0xFFFFFFFF), np.uint64(CR_SCE_SITE))
    j = np.arange(N, dtype=np.uint64)
    x = fmix32((key + j * np.uint64(CR_PHI)) & M32)
    return (1 + ((x * np.uint64(V - 1)) >> np.uint64(32))).astype(np.int32)
