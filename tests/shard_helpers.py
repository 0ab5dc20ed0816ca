"""Shared by the shard-exchange tests (CPU gloo and ranks-on-one-GPU): seeded per-rank gradients and the
reference's rank loop (hp:356-394) from the oracle, held to the gather exchange's bars.  TEST INFRASTRUCTURE."""
import numpy as np
import torch

from helpers import rel_err
from oracle import hdpissa_oracle as O


def seeded_grads(L, j, rank, step):
    """The per-rank gradients of tests/test_gpu_ranks_one_gpu.py."""
    g = torch.Generator().manual_seed(1000 * step + 10 * j + rank)
    return (torch.randn(L.A.shape, generator=g) * 1e-14, torch.randn(L.B.shape, generator=g) * 1e-14)


class OracleRanks:
    """Runs the oracle's Adam and rank loop beside the product for every module and holds the product's W
    to it after each step: float32 merged W 1e-5 and update 1e-4 against ``O.delta_w_exact``; bf16 update
    2e-2 with < 2 % of elements differing from ``O.merge(O.delta_w(...))``.  ``figures`` keeps the worst
    measured values."""

    def __init__(self, layers, wn, r, dt, lr):
        self.layers, self.wn, self.r, self.dt, self.lr = layers, wn, r, dt, lr
        z = lambda *s: np.zeros(s, np.float32)  # noqa: E731
        self.mv = {(i, j): ([z(r, L.in_features), z(L.out_features, r)], [z(r, L.in_features), z(L.out_features, r)])
                   for i in range(wn) for j, L in enumerate(layers)}
        W0 = [L.W_res.float().cpu().numpy() for L in layers]
        self.Wref = [w.astype(np.float64) if dt == torch.float32 else w for w in W0]
        self.figures = dict(w=0.0, upd=0.0, diff=0.0)

    def deltas(self, step):
        """Every rank's (dA, dB) of this step per module (advances the oracle's Adam moments)."""
        out = []
        for j, L in enumerate(self.layers):
            dA, dB = [], []
            for i in range(self.wn):
                gA, gB = (x.numpy() for x in seeded_grads(L, j, i, step))
                (mA, mB), (vA, vB) = self.mv[(i, j)]
                mA, vA, da = O.adam_factors(gA, mA, vA, step, self.lr)
                mB, vB, db = O.adam_factors(gB, mB, vB, step, self.lr)
                self.mv[(i, j)] = ([mA, mB], [vA, vB])
                dA.append(da)
                dB.append(db)
            out.append((dA, dB))
        return out

    def check(self, step, deltas, Ws):
        """``Ws``: the product's merged W per module after ``step`` (float tensors on the host)."""
        r, wn, f = self.r, self.wn, self.figures
        for j, (L, (dA, dB)) in enumerate(zip(self.layers, deltas)):
            fa = L._arena.fac_all
            A = [fa[i][L._oa:L._oa + r * L.in_features].view(r, -1).cpu().numpy() for i in range(wn)]
            B = [fa[i][L._ob:L._ob + L.out_features * r].view(-1, r).cpu().numpy() for i in range(wn)]
            got = Ws[j].numpy()
            if self.dt == torch.float32:
                exact = O.delta_w_exact(dA, dB, A, B)
                prev = self.Wref[j]
                ew, eu = rel_err(got, prev + exact), rel_err(got - prev, exact)
                f["w"], f["upd"] = max(f["w"], ew), max(f["upd"], eu)
                assert ew < 1e-5, (step, j, ew)
                assert eu < 1e-4, (step, j, eu)
                self.Wref[j] = got.astype(np.float64)  # continue from the product's W (the next step's input)
            else:
                ref = O.merge(self.Wref[j], O.delta_w(dA, dB, A, B, "bfloat16"), "bfloat16")
                upd = rel_err(got - self.Wref[j], ref - self.Wref[j])
                diff = float(np.mean(got != ref))
                f["upd"], f["diff"] = max(f["upd"], upd), max(f["diff"], diff)
                assert upd < 2e-2 and diff < 0.02, (step, j, upd, diff)
                self.Wref[j] = got
