"""Plain bf16 against the fp64 oracle, per parameter.

  python tools/probes/bf16_vs_oracle.py envelope     every shape of tests/bf16_ref.SHAPES (+ the plain-bf16 small-shape and wide cases
                                                     of tests/test_model_gpu.py): the launch plan, then for every parameter the kernel's
                                                     error (of the parameter's own largest gradient), the rounding model's E_k, their
                                                     ratio, the bound 3 E_k + 2e-3 and the error's share of it.  profiles/bf16_envelope.txt
                                                     is one run of this.  No test takes a number from that file.
  python tools/probes/bf16_vs_oracle.py              T 200 / D 50: each parameter's error relative to its own largest gradient, for the
                                                     one-launch block backward and for the tile kernels (CASTREC_NO_STACK_BWD)."""
import os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
import castrec_amd.engine as E
from oracle import fpmodel as fm
import bf16_ref as br
from test_model_gpu import make_batch, oracle_drop, oracle_with_engine_gates, _other_shapes


def envelope_table():
    cases = [(s, dict(dropout=0.2, n_slabs=7 if s[1] <= 64 else 5)) for s in br.SHAPES]
    # test_wide_row_kernels' two plain-bf16 cases at their own draw and dropout
    cases += [(("cast_1", 128, 2, 37, 3, 2, 0), {}), (("sasrec", 256, 4, 50, 5, 1, 0), {})]
    for (model, D, H, T, B, L, draw), kw in cases:
        rep = []
        verdict = "within the bounds"
        try:
            _other_shapes(E, model, D, H, T, L, B=B, prec="bf16", draw=draw, report=rep, **kw)
        except AssertionError as e:
            verdict = "OUTSIDE: %s" % (str(e).splitlines() or ["?"])[0][:200]
        r = rep[0]
        eng = r["eng"]
        print("== %s D %d H %d T %d B %d L %d draw %d %s: %s" % (model, D, H, T, B, L, draw, kw, verdict))
        print("   forward :", " ".join(n for n, _, _ in eng.fwd))
        print("   backward:", " ".join(n for n, _, _ in eng.bwd))
        print("   loss error %.3g (E_loss %.3g, bound %.3g)   forward rows %.3g (E_act %.3g, bound %.3g)"
              % (r["loss"][0], r["env"][2], r["loss"][1], r["act"][0], r["env"][1], r["act"][1]))
        print("   %-22s %10s %10s %8s %10s %7s" % ("parameter", "error", "E_k", "err/E_k", "bound", "share"))
        for share, k, err, Ek, bound in r["grads"]:
            print("   %-22s %10.3g %10.3g %8.2f %10.3g %7.2f" % (k, err, Ek, err / max(Ek, 1e-30), bound, share))
        sys.stdout.flush()


def headline():
    B, T, D, H = int(os.environ.get("PB", 3)), int(os.environ.get("PT", 200)), 50, 1
    for prec in ("bf16", "bf16x3"):
        for name, env in (("block", None), ("tile", "CASTREC_NO_STACK_BWD")):
            rs = np.random.RandomState(5)
            hp = E.Hyper(maxlen=T, hidden_units=D, num_blocks=2, num_heads=H, dropout_rate=0.2, max_bins=9, num_context_blocks=1, lr=1e-3, seed=13)
            ohp = fm.Hyper(maxlen=T, hidden_units=D, num_blocks=2, num_heads=H, dropout_rate=0.2, max_bins=9, num_context_blocks=1, lr=1e-3)
            if env:
                os.environ[env] = "1"
            eng = E.Engine("cast_1", 9, 45, hp, B, training=True, n_slabs=7, attn_precision=prec)
            if env:
                del os.environ[env]
            if os.environ.get("PINIT") == "engine":                   # the perturbation of test_register_layout_kernels_equal_the_tile_kernels
                eng.P.add_(0.05 * torch.randn(eng.P.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)))
            else:
                P = fm.init_params("cast_1", 9, 45, ohp, seed=8)
                P = {k: v + 0.05 * torch.tensor(rs.standard_normal(tuple(v.shape))) for k, v in P.items()}
                eng.load_params(P)
            P = {k: v.double().cpu() for k, v in eng.get_params().items()}
            batch = make_batch(rs, B, T, 45, 9)
            eng.set_batch(*batch)
            eng.launch_step(apply=False)
            torch.cuda.synchronize()
            drop = oracle_drop(E, 13, 1, 0.2, B, T, H)
            out, G = oracle_with_engine_gates(eng, B, T, drop, prec, lambda: fm.loss_and_grads("cast_1", P, ohp, fm.to_batch(*batch), drop))
            got = eng.grads()
            errs = sorted(((float((got[k].cpu().double() - G[k]).abs().max() / max(float(G[k].abs().max()), 1e-12)), k) for k in G if not k.endswith(".bk")), reverse=True)
            for k in ("ctx_time.1.w2", "trunk.0.w2", "ctx_time.1.w1"):
                print("      ", k, "own max %.4f  error %.4f;  hid max %s" % (float(G[k].abs().max()), float((got[k].cpu().double() - G[k]).abs().max()),
                      ["%s %.2f" % (n, float(b.abs().max())) for n, b in eng._bufs.items() if n.endswith(".hid")]))
            print(prec, name, "loss", float(eng.state[0] / eng.state[2]), float(out["loss"]), "  worst (error / own max):", ["%s %.3g" % (k, e) for e, k in errs[:8]])


if __name__ == "__main__":
    if sys.argv[1:] == ["envelope"]:
        envelope_table()
    else:
        headline()
