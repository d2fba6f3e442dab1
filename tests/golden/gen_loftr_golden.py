"""Writes tests/golden/loftr_*.npz: float64 results of tests/loftr_reference.py on the pairs of tests/golden/loftr_cases.py.

    python -m tests.golden.gen_loftr_golden

Results only (the inputs are regenerated from the seeds).  The generator asserts what the cases are for and refuses to write
otherwise:
  * every selection decision of the float64 result, at every threshold a fixture holds, has a margin above 10 x TOL_CONF
    (`decisions_hold`: the gaps between a candidate and the threshold, and from the row and the column maximum to their
    runners-up).  A device result within TOL_CONF of the float64 one then takes the same decisions: the tests compare the index
    sets exactly, no pair excused;
  * the parallel (quirk q6) schedule differs from the sequential one by more than 100 x TOL_CONF somewhere in conf_matrix;
  * at THR, in the leading and in the trailing border band of each of the two grids there is a pair with conf > thr and mutual
    maximum that the border alone removes;
  * float32 on the CPU selects the same sets; its distance in conf_matrix is printed.
"""
import os

import numpy as np
import torch

from tests import loftr_reference as R
from tests.golden.loftr_cases import LOFTR_PAIRS, VARIANTS, WINDOWS, THR, loftr_cfg, loftr_pair, loftr_state_dict
from tests.helpers import TOL_CONF

HERE = os.path.dirname(os.path.abspath(__file__))


def decisions_hold(conf, hw0, hw1, thr, b, m):
    """True when every row's outcome survives a perturbation of every confidence by less than m / 2: the cells within m of the row
    maximum are either all out (in a border band, below thr - m, or below another entry of their column by more than m), or there
    is one such cell and it is in (inside both borders, above thr + m, above the rest of its column by more than m)."""
    c = conf[0]
    inb = R.border_mask(hw0, hw1, b)
    top = c.topk(2, dim=0)
    rows = torch.arange(c.shape[0])[:, None]
    other = torch.where(top.indices[0][None, :] == rows, top.values[1][None, :], top.values[0][None, :])
    near = c > c.max(dim=1, keepdim=True)[0] - m
    out = ~inb | (c < thr - m) | (other - c > m)
    sel = inb & (c > thr + m) & (c - other > m)
    ok = (near & ~out).sum(1) == 0
    ok |= (near.sum(1) == 1) & (near & sel).any(1)
    return bool(ok.all())


def decision_margin(conf, hw0, hw1, thr, b):
    """the largest m (to 2 %) at which decisions_hold"""
    lo, hi = 0.0, 0.5
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        if decisions_hold(conf, hw0, hw1, thr, b, mid):
            lo = mid
        else:
            hi = mid
    return lo


def border_only_pairs(conf, hw0, hw1, thr, b):
    """pairs with conf > thr and mutual maximum, per (grid, end) band that holds one of their cells"""
    i, j, _ = R.select(conf, hw0, hw1, thr, 0)
    iy, ix, jy, jx = i // hw0[1], i % hw0[1], j // hw1[1], j % hw1[1]
    lead0, trail0 = (iy < b) | (ix < b), (iy >= hw0[0] - b) | (ix >= hw0[1] - b)
    lead1, trail1 = (jy < b) | (jx < b), (jy >= hw1[0] - b) | (jx >= hw1[1] - b)
    return [int(x.sum()) for x in (lead0, trail0, lead1, trail1)]


def main():
    sd = loftr_state_dict()
    torch.manual_seed(0)
    for name in LOFTR_PAIRS:
        out = {}
        base = loftr_pair(name)
        cfg = loftr_cfg()
        r64 = R.forward(sd, base, cfg, enable_fine=False)
        conf = r64["conf_matrix"]
        par = R.forward(sd, base, cfg, enable_fine=False, sequential=False)["conf_matrix"]
        r32 = R.forward(sd, base, cfg, enable_fine=False, dtype=torch.float32)
        d_par = float((par - conf).abs().max())
        d32 = float((r32["conf_matrix"].double() - conf).abs().max())
        assert d_par > 100 * TOL_CONF, (name, "parallel schedule too close", d_par)
        bands = border_only_pairs(conf, r64["hw0_c"], r64["hw1_c"], THR, cfg["match_coarse"]["border_rm"])
        assert min(bands) >= 1, (name, "a border band removes nothing", bands)
        out["conf_matrix"] = conf[0].numpy().astype(np.float32)
        line = []
        for vname, (thr, _) in VARIANTS.items():
            margin = decision_margin(conf, r64["hw0_c"], r64["hw1_c"], thr, cfg["match_coarse"]["border_rm"])
            assert margin > 10 * TOL_CONF, (name, vname, "marginal decision", margin)
            data = loftr_pair(name, vname)
            for W in WINDOWS:
                r = R.forward(sd, data, loftr_cfg(thr, W))
                i32, j32, _ = R.select(r32["conf_matrix"], r64["hw0_c"], r64["hw1_c"], thr, cfg["match_coarse"]["border_rm"])
                assert torch.equal(i32, r["i_ids"]) and torch.equal(j32, r["j_ids"]), (name, vname, "float32 selects another set")
                p = "%s/w%d/" % (vname, W)
                for k in ("i_ids", "j_ids", "mconf", "mkpts0_c", "mkpts1_c", "mkpts1_f", "expec_f"):
                    out[p + k] = r[k].numpy()
            line.append("%s: M %d margin %.3g" % (vname, len(r["i_ids"]), margin))
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
        print("%s  |conf64 - conf32| %.3g  |sequential - parallel| %.3g  border-only pairs (lead0, trail0, lead1, trail1) %s\n    %s"
              % (name, d32, d_par, bands, "; ".join(line)))


if __name__ == "__main__":
    main()
