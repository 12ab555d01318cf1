"""Times cr_score_topk (full-catalogue top-K, csrc/cr_topk.hip) with HIP events at the shapes of DESIGN.md "Full-catalogue top-K",
against the HBM and MFMA roofs, beside torch.matmul (fp32) + torch.topk where the [B, V] score matrix fits.

    python tools/topk_bench.py [--shapes a,b,c,d] [--reps 5] [--out DIR/topk_bench.json] [--no-torch]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import castrec_amd  # noqa: E402,F401
from castrec_amd import lib as L  # noqa: E402
from castrec_amd import ops as O  # noqa: E402

SHAPES = {"a": ("ml-1m", 3416, 50, 6040, 10), "b": ("C4 vocabulary", 368000, 128, 10000, 10),
          "c": ("C5 table, 128 users", 10 ** 7, 256, 128, 100), "d": ("C5 table, 1024 users", 10 ** 7, 256, 1024, 100)}
HBM = 8.0e12                      # bytes / s (spec)
BF16_PEAK = 2.5e15                # dense bf16 MFMA FLOP / s (spec)


def _time(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e-3)
    out.sort()
    return out[len(out) // 2], out


def run(key, reps, with_torch):
    name, V, D, B, K = SHAPES[key]
    g = torch.Generator(device="cuda").manual_seed(0)
    table = torch.randn(V, D, device="cuda", generator=g) * 0.05
    q = torch.randn(B, D, device="cuda", generator=g)
    ws = torch.empty(O.topk_workspace_bytes(B, V, D, K), dtype=torch.uint8, device="cuda")
    ids = torch.empty(B, K, dtype=torch.int32, device="cuda")
    sc = torch.empty(B, K, dtype=torch.float32, device="cuda")
    fn = lambda: O.score_topk(q, D, table, B, K, L.PREC_BF16X3, None, None, None, ws, ids, sc)
    t, all_t = _time(fn, reps)
    nbytes = V * D * 4 + B * D * 4 + B * K * 8
    flop = 2.0 * B * V * D * 3
    t_hbm, t_mfma = nbytes / HBM, flop / BF16_PEAK
    bound = "hbm" if t_hbm >= t_mfma else "mfma"
    r = dict(shape=key, name=name, V=V, D=D, B=B, K=K, time_s=t, times_s=all_t, hbm_bytes=nbytes, hbm_roof_s=t_hbm,
             hbm_fraction=t_hbm / t, mfma_flop_bf16x3=flop, mfma_roof_s=t_mfma, mfma_fraction=t_mfma / t, binding=bound,
             binding_fraction=max(t_hbm, t_mfma) / t, workspace_bytes=ws.numel())
    if with_torch and B * V * 4 <= 48 * 2 ** 30:
        def base():
            s = q @ table.t()
            s[:, 0] = -float("inf")
            return torch.topk(s, K, dim=1)
        try:
            tb, _ = _time(base, max(2, reps // 2), warm=1)
            r.update(torch_matmul_topk_s=tb, speedup_vs_torch=tb / t)
            bs = base()
            ref = bs.indices.to(torch.int32)
            r["agree_with_torch_ids"] = float((ref == ids).float().mean())
        except RuntimeError as e:                         # (out of memory: reported, not fatal)
            r["torch_error"] = str(e)[:200]
        torch.cuda.empty_cache()
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c,d")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    res = [run(k, a.reps, not a.no_torch) for k in a.shapes.split(",")]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), results=res), f, indent=1)


if __name__ == "__main__":
    main()
