"""Training fixtures of the full-attention configuration, produced by running the REFERENCE (imported read-only through
oracle/refload.py) in train() mode on the seeded inputs of tests/golden/fullattn_train_cases.py.  Runs only where the reference is:

    python tests/golden/gen_full_attention_train_golden.py

Writes tests/golden/fullattn*_train_*.npz with the contents of tests/golden/gen_golden.py gen_train: the outputs of the train()-mode
forward, the recorded torch.randint draws of its training branch, the gradient digest (sum, L2 norm) of every parameter and the whole
GRAD_TENSORS gradients of the fixed scalar of tests/helpers.py train_loss_weights (the reference's own autograd), and the BatchNorm running
statistics after one forward.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle.refload import load_reference_model_class  # noqa: E402
from tests.golden.cases import GOLDEN_CPU_THREADS  # noqa: E402
from tests.golden.gen_golden import conf_digest_batched  # noqa: E402
from tests.golden.fullattn_train_cases import FULLATTN_TRAIN_CASES, train_setup  # noqa: E402
from tests.helpers import train_loss_weights, GRAD_TENSORS  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def _run(cls, cfg, sd, data, draws=None, grad=False):
    """train()-mode forward of the reference; draws = None records the torch.randint draws, else replays them"""
    model = cls(cfg)
    model.load_state_dict(sd, strict=True)
    model.train()
    n_full = sum(type(m).__name__ == "FullAttention" for m in model.modules())
    real = torch.randint
    rec = []
    replay = [x.clone() for x in draws] if draws is not None else None

    def randint(*a, **kw):
        if replay is not None:
            return replay.pop(0)
        x = real(*a, **kw)
        rec.append(x.clone())
        return x
    torch.manual_seed(123)
    torch.randint = randint
    try:
        with torch.set_grad_enabled(grad):
            model(data)
    finally:
        torch.randint = real
    return model, rec, n_full


def gen_train():
    cls = load_reference_model_class()
    for name, (_, (coarse, fine)) in FULLATTN_TRAIN_CASES.items():
        cfg, sd, data = train_setup(name)
        model, draws, n_full = _run(cls, cfg, sd, data)
        want = (len(cfg["loftr_coarse"]["layer_names"]) * cfg["loftr_coarse"]["layer_iter_n"] if coarse else 0) + \
               (len(cfg["loftr_fine"]["layer_names"]) * cfg["loftr_fine"]["layer_iter_n"] if fine else 0)
        assert n_full == want, (name, n_full, want)
        out = {k: data[k].numpy() for k in ["b_ids", "i_ids", "j_ids", "gt_mask", "m_bids", "mkpts_3d_db", "mkpts_query_c", "mconf", "expec_f",
                                             "mkpts_query_f"]}
        out.update(conf_digest_batched(data["conf_matrix"]))
        out["meta"] = np.array([data["bs"], *data["q_hw_i"], *data["q_hw_c"], *data["q_hw_f"], data.get("W", -1)], dtype=np.int64)
        for i, d in enumerate(draws):
            out["randint_%d" % i] = d.numpy()
        out["n_randint"] = np.array(len(draws))
        d2 = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in train_setup(name)[2].items()}
        model2, _, _ = _run(cls, cfg, sd, d2, draws, grad=True)
        wc, we = train_loss_weights(d2["conf_matrix"].shape, d2["expec_f"].shape)
        ((d2["conf_matrix"] * wc).sum() + (d2["expec_f"] * we).sum()).backward()
        gnames = [n for n, p_ in model2.named_parameters() if p_.grad is not None]
        out["grad_names"] = np.array(gnames)
        out["grad_digest"] = np.array([[float(model2.get_parameter(n).grad.double().sum()),
                                        float(model2.get_parameter(n).grad.double().norm())] for n in gnames])
        for n in GRAD_TENSORS:
            out["grad/" + n] = model2.get_parameter(n).grad.numpy()
        for n in gnames:
            if n.startswith(("loftr_coarse.", "loftr_fine.")):
                assert float(model2.get_parameter(n).grad.abs().max()) > 0, n
        for k, v in model.state_dict().items():          # running statistics after ONE training forward
            if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
                out["bn/" + k] = v.numpy()
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **out)
        print(name, "M' =", len(data["b_ids"]), "M =", len(data["mconf"]), "draws", [tuple(d.shape) for d in draws], "grads", len(gnames),
              "bytes", os.path.getsize(path))


if __name__ == "__main__":
    torch.set_num_threads(GOLDEN_CPU_THREADS)
    gen_train()
