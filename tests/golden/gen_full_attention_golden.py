"""Fixtures of the full-attention configuration (`attention: "full"` in loftr_coarse and loftr_fine, which builds FullAttention
upstream: transformer.py:32-40, linear_attention.py:64-95), produced by running the REFERENCE (/root/reference, imported read-only
through oracle/refload.py) on the seeded inputs of tests/golden/fullattn_cases.py.  Runs only where the reference is:

    python tests/golden/gen_full_attention_golden.py

Writes tests/golden/fullattn_*.npz: loftr_coarse-alone digests (tests/helpers.py transformer_digest) and whole-model outputs in the
digest format of the existing e2e / batch fixtures.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle.refload import load_reference_model_class  # noqa: E402
from tests.golden.cases import GOLDEN_CPU_THREADS  # noqa: E402
from tests.helpers import transformer_digest  # noqa: E402
from tests.golden.gen_golden import e2e_outputs, conf_digest_batched  # noqa: E402
from tests.golden.fullattn_cases import (FULLATTN_TRANSFORMER_CASES, FULLATTN_E2E_CASES, FULLATTN_BATCH_CASES,  # noqa: E402
                                         fullattn_transformer_setup, fullattn_e2e_setup, fullattn_batch_setup)

HERE = os.path.dirname(os.path.abspath(__file__))
PEAKED_SHARE = 0.5     # the sharp case must have most softmax row maxima above 0.5


def _row_max_recorder(model):
    """forward hooks on every FullAttention of loftr_coarse: the largest softmax probability of each query row, per head"""
    maxima = []

    def hook(mod, args, out):
        q, k = args[0], args[1]
        logits = torch.einsum("nlhd,nshd->nlsh", q, k) / q.size(3) ** 0.5
        maxima.append(torch.softmax(logits, dim=2).max(2).values.flatten())

    handles = [m.register_forward_hook(hook) for n, m in model.loftr_coarse.named_modules() if type(m).__name__ == "FullAttention"]
    assert handles, "no FullAttention module in loftr_coarse"
    return maxima, handles


def gen_transformer():
    cls = load_reference_model_class()
    for name, (L, n, seed, factor) in FULLATTN_TRANSFORMER_CASES.items():
        cfg, sd, tokens2d, bank = fullattn_transformer_setup(name)
        model = cls(cfg).eval()
        model.load_state_dict(sd, strict=True)
        maxima, handles = _row_max_recorder(model)
        with torch.no_grad():
            f3, f2 = model.loftr_coarse(bank, tokens2d)
        for h in handles:
            h.remove()
        share = float((torch.cat(maxima) > 0.5).float().mean())
        print(name, "q/k factor %.1f: share of softmax rows with max > 0.5 = %.3f" % (factor, share))
        if factor != 1.0 and share < PEAKED_SHARE:
            raise SystemExit("%s: softmax not peaked enough (%.3f < %.2f): raise the q/k factor" % (name, share, PEAKED_SHARE))
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **transformer_digest(f3[0], f2[0]))


def gen_e2e():
    cls = load_reference_model_class()
    for name in FULLATTN_E2E_CASES:
        cfg, sd, data = fullattn_e2e_setup(name)
        model = cls(cfg).eval()
        model.load_state_dict(sd, strict=True)
        with torch.no_grad():
            model(data)
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **e2e_outputs(data))
        print(name, "M =", len(data["mconf"]))


def gen_batch():
    cls = load_reference_model_class()
    for name in FULLATTN_BATCH_CASES:
        cfg, sd, data = fullattn_batch_setup(name)
        model = cls(cfg).eval()
        model.load_state_dict(sd, strict=True)
        with torch.no_grad():
            model(data)
        out = {k: data[k].numpy() for k in ["b_ids", "i_ids", "j_ids", "gt_mask", "m_bids", "mkpts_3d_db", "mkpts_query_c", "mconf",
                                             "expec_f", "mkpts_query_f"]}
        out.update(conf_digest_batched(data["conf_matrix"]))
        out["meta"] = np.array([data["bs"], *data["q_hw_i"], *data["q_hw_c"], *data["q_hw_f"], data.get("W", -1)], dtype=np.int64)
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
        print(name, "M =", len(data["mconf"]))


if __name__ == "__main__":
    torch.set_num_threads(GOLDEN_CPU_THREADS)
    gen_transformer()
    gen_e2e()
    gen_batch()
