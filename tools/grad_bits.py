"""Comparison aid for a change that must not move a bit of the gradients: `actor_backward` and `critic_backward` on seeded networks
and rows, every result into ONE .npz.  Run it in a fresh process with each of two builds of the library (each from its own tree) and
compare the two files array by array, byte for byte:

    python tools/grad_bits.py a.npz                  # in tree A
    python tools/grad_bits.py b.npz                  # in tree B
    python tools/grad_bits.py --compare a.npz b.npz  # anywhere: prints the count, exits 1 on the first difference

The cases: tanh / relu x feature LayerNorm on / off x rows 1, 17, 65, 16 401 and 70 000 (the last a multi-pass grid with a ragged
tail) x dent 0 / -0.002 for each of three agents' actors (`ActorGrads.flat`, `sq_norm`), and the critic of the same activation and
feature LayerNorm per row count (`CriticGrads.flat`, `sq_norm`)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ROWS = (1, 17, 65, 16401, 70000)
DENTS = (0.0, -0.002)


def network(rng, n_in, n_out, feature_norm, names):
    """every member random and non-zero (torch's Linear bounds, LayerNorm gains about 1) under the params struct's field names"""
    u = lambda shape, fan_in: ((rng.random(shape) * 2 - 1) / np.sqrt(fan_in)).astype(np.float32)
    g, b = names
    p = {"w1": u((64, n_in), n_in), "b1": u((64,), n_in), "w2": u((64, 64), 64), "b2": u((64,), 64),
         "w3": u((n_out, 64) if n_out > 1 else (64,), 64), "b3": u((n_out,), 64) if n_out > 1 else float(u((1,), 64)[0])}
    for k, n in (("ln0", n_in), ("ln1", 64), ("ln2", 64)):
        if k == "ln0" and not feature_norm:
            continue
        p[k + g] = (1.0 + 0.2 * rng.standard_normal(n)).astype(np.float32)
        p[k + b] = (0.2 * rng.standard_normal(n)).astype(np.float32)
    return p


def compare(a, b):
    x, y = np.load(a), np.load(b)
    assert sorted(x.files) == sorted(y.files), "the two files hold different cases"
    for k in sorted(x.files):
        if x[k].dtype != y[k].dtype or x[k].shape != y[k].shape or x[k].tobytes() != y[k].tobytes():
            print("DIFFERS", k, int((x[k].view(np.uint8) != y[k].view(np.uint8)).sum()), "bytes")
            return 1
    print(len(x.files), "arrays compared, none differs")
    return 0


def main(out_path):
    import torch

    import bench
    eng, _, _ = bench.build_engine(8, 672, 0, seed=99, debug_flags=0)
    dev, out = eng.device, {}
    g = torch.Generator().manual_seed(11)
    obs = torch.randn((max(ROWS), 26), generator=g).to(dev)
    share = torch.randn((max(ROWS), 29), generator=g).to(dev)
    actions = torch.randint(0, 3, (max(ROWS),), generator=g, dtype=torch.int32).to(dev)
    coef = (torch.randn((max(ROWS),), generator=g) / 64).to(dev)
    for activation in ("tanh", "relu"):
        for fn in (True, False):
            rng = np.random.default_rng(1000 + 10 * (activation == "relu") + fn)
            for agent in range(3):
                eng.set_actor(agent, dict(network(rng, 26, 3, fn, ("_gamma", "_beta")), activation=activation))
            eng.set_critic(network(rng, 29, 1, fn, ("_g", "_b")), None, activation)
            for n in ROWS:
                tag = f"{activation}_ln0{int(fn)}_n{n}"
                for agent in range(3):
                    for dent in DENTS:
                        r = eng.actor_backward(agent, obs[:n].contiguous(), actions[:n].contiguous(), coef[:n].contiguous(), dent)
                        out[f"actor{agent}_{tag}_dent{int(dent != 0)}_flat"] = r.flat.cpu().numpy()
                        out[f"actor{agent}_{tag}_dent{int(dent != 0)}_sq"] = r.sq_norm.cpu().numpy()
                r = eng.critic_backward(share[:n].contiguous(), coef[:n].contiguous())
                out[f"critic_{tag}_flat"] = r.flat.cpu().numpy()
                out[f"critic_{tag}_sq"] = r.sq_norm.cpu().numpy()
    assert all(np.isfinite(v).all() for v in out.values()) and all(np.abs(v).max() > 0 for v in out.values())
    np.savez(out_path, **out)
    print(len(out), "arrays ->", out_path, flush=True)
    eng.close()


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
