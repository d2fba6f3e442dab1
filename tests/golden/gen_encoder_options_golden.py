"""Fixtures of the encoder options (rezero, in-layer instancenorm, feat_norm_method none, keypoint-encoder layernorm; case table in
tests/golden/encopt_cases.py), produced by running the REFERENCE (imported read-only through oracle/refload.py) on seeded inputs.
Runs only where the reference is:

    python tests/golden/gen_encoder_options_golden.py

Writes tests/golden/encopt_*.npz in the digest formats of the existing fixtures (`e2e_outputs`, `conf_digest_batched`, the training
digests of gen_golden.gen_train) and the reference's state-dict contract of every variant.

Fixtures with `feat_norm_method: none`: the logits are C = 256 times larger, the softmaxes saturate, and two correct fp32 evaluations
differ by more than 1e-4 in conf_matrix.  For these the reference also runs in float64 (`model.double()`, double inputs); the float64
outputs are the golden, and `ref_fp32_err` = max |conf_matrix(fp32) - conf_matrix(fp64)| of the reference's own two runs is stored with
them (the GPU bar on conf_matrix / mconf is max(1e-4, 2 * ref_fp32_err): both implementations accumulate in fp32, in different orders).
The two runs must select the same (i_ids, j_ids) -- otherwise index equality would be an unfair demand -- and the golden must hold a
confidence above 0.99."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle.refload import load_reference_model_class  # noqa: E402
from tests.golden.cases import GOLDEN_CPU_THREADS  # noqa: E402
from tests.golden.gen_golden import e2e_outputs, conf_digest_batched  # noqa: E402
from tests.golden import encopt_cases as EC  # noqa: E402
from onepose_plus_plus_amd.config import default_config  # noqa: E402
from onepose_plus_plus_amd.synthetic import make_state_dict  # noqa: E402
from tests.helpers import train_loss_weights  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MATCH_KEYS = ["b_ids", "i_ids", "j_ids", "gt_mask", "m_bids", "mkpts_3d_db", "mkpts_query_c", "mconf", "expec_f", "mkpts_query_f"]


def _to(data, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else (v.clone() if torch.is_tensor(v) else v))
            for k, v in data.items()}


def _model(cls, cfg, sd, dtype=torch.float32):
    model = cls(cfg)
    model.load_state_dict(sd, strict=True)
    return model.to(dtype)


def _eval_run(cls, cfg, sd, data, dtype):
    d = _to(data, dtype)
    with torch.no_grad():
        _model(cls, cfg, sd, dtype).eval()(d)
    return d


def _fp64_golden(cls, cfg, sd, data, name):
    """-> (float64 run, ref_fp32_err); asserts what the module docstring demands of a feat_norm none fixture"""
    d32, d64 = _eval_run(cls, cfg, sd, data, torch.float32), _eval_run(cls, cfg, sd, data, torch.float64)
    for k in ("b_ids", "i_ids", "j_ids"):
        if not torch.equal(d32[k], d64[k]):
            raise SystemExit("%s: the fp32 and fp64 reference runs select different %s: change the input seed" % (name, k))
    err = float((d32["conf_matrix"].double() - d64["conf_matrix"]).abs().max())
    top = float(d64["mconf"].max()) if len(d64["mconf"]) else 0.0
    print("%s: ref_fp32_err = %.3e, M = %d, max conf = %.6f" % (name, err, len(d64["mconf"]), top))
    if top <= 0.99:
        raise SystemExit("%s: no confidence above 0.99 in the golden" % name)
    return d64, err


def _f32_arrays(out):
    """float64 results are stored as float32 (the nearest fp32 to the fp64 value: half an ulp, far below every bar)"""
    return {k: (v.astype(np.float32) if v.dtype == np.float64 else v) for k, v in out.items()}


def gen_contract():
    cls = load_reference_model_class()
    out = {}
    for v, settings in EC.VARIANTS.items():
        cfg = EC.encopt_config(default_config(), settings)
        ref = cls(cfg)
        sd = ref.state_dict()
        ref.load_state_dict(make_state_dict(cfg, 0), strict=True)       # a synthetic state dict of that config strict-loads upstream
        ndim = max(t.dim() for t in sd.values())
        out[v + "/keys"] = np.array(list(sd))
        out[v + "/shapes"] = np.array([list(t.shape) + [-1] * (ndim - t.dim()) for t in sd.values()], dtype=np.int64)
        print("contract", v, len(sd), "tensors")
    np.savez_compressed(os.path.join(HERE, EC.MODULE_CONTRACT + ".npz"), **out)


def gen_e2e():
    cls = load_reference_model_class()
    for table, setup in ((EC.ENCOPT_E2E_CASES, EC.e2e_setup), (EC.ENCOPT_FULLATTN_CASES, EC.fullattn_setup)):
        for name in table:
            cfg, sd, data = setup(name)
            if cfg["coarse_matching"]["feat_norm_method"] != "sqrt_feat_dim":
                d, err = _fp64_golden(cls, cfg, sd, data, name)
                out = _f32_arrays(e2e_outputs(d))
                out["ref_fp32_err"] = np.array(err)
            else:
                d = _eval_run(cls, cfg, sd, data, torch.float32)
                out = e2e_outputs(d)
                print(name, "M =", len(d["mconf"]))
            assert len(d["mconf"]) > 0, name
            np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)


def _batched_outputs(d):
    out = {k: d[k].numpy() for k in MATCH_KEYS}
    out.update(conf_digest_batched(d["conf_matrix"]))
    out["meta"] = np.array([d["bs"], *d["q_hw_i"], *d["q_hw_c"], *d["q_hw_f"], d.get("W", -1)], dtype=np.int64)
    return out


def gen_batch():
    cls = load_reference_model_class()
    for name in EC.ENCOPT_BATCH_CASES:
        cfg, sd, data = EC.batch_setup(name)
        d, err = _fp64_golden(cls, cfg, sd, data, name)
        out = _f32_arrays(_batched_outputs(d))
        out["ref_fp32_err"] = np.array(err)
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
        print(name, "per sample:", torch.bincount(d["b_ids"], minlength=int(d["bs"])).tolist())


def _train_run(cls, cfg, sd, data, dtype, draws=None, grad=False):
    """train()-mode forward of the reference; draws = None records the torch.randint draws, else replays them"""
    model = _model(cls, cfg, sd, dtype)
    model.train()
    d = _to(data, dtype)
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
            model(d)
    finally:
        torch.randint = real
    return model, d, rec


def gen_train():
    """as gen_golden.gen_train; the feat_norm none rule of the module docstring applies to the forward outputs (float64 golden), the
    gradients are the reference's own float64 autograd on the same draws"""
    cls = load_reference_model_class()
    for name in EC.ENCOPT_TRAIN_CASES:
        cfg, sd, data = EC.train_setup(name)
        model, d, draws = _train_run(cls, cfg, sd, data, torch.float64)
        _, d32, _ = _train_run(cls, cfg, sd, data, torch.float32, draws)
        for k in ("b_ids", "i_ids", "j_ids"):
            if not torch.equal(d32[k], d[k]):
                raise SystemExit("%s: the fp32 and fp64 reference runs select different %s: change the input seeds" % (name, k))
        err = float((d32["conf_matrix"].double() - d["conf_matrix"]).abs().max())
        print("%s: ref_fp32_err = %.3e, max conf = %.6f" % (name, err, float(d["mconf"].max())))
        out = _f32_arrays(_batched_outputs({k: (v.detach() if torch.is_tensor(v) else v) for k, v in d.items()}))
        out["ref_fp32_err"] = np.array(err)
        for i, x in enumerate(draws):
            out["randint_%d" % i] = x.numpy()
        out["n_randint"] = np.array(len(draws))
        model2, d2, _ = _train_run(cls, cfg, sd, data, torch.float64, draws, grad=True)
        wc, we = train_loss_weights(d2["conf_matrix"].shape, d2["expec_f"].shape)
        ((d2["conf_matrix"] * wc.double()).sum() + (d2["expec_f"] * we.double()).sum()).backward()
        gnames = [n for n, p_ in model2.named_parameters() if p_.grad is not None]
        out["grad_names"] = np.array(gnames)
        out["grad_digest"] = np.array([[float(model2.get_parameter(n).grad.sum()), float(model2.get_parameter(n).grad.norm())] for n in gnames])
        for n in EC.train_grad_tensors(cfg):
            g = model2.get_parameter(n).grad
            assert float(g.abs().max()) > 0, n
            out["grad/" + n] = g.float().numpy()
        assert not any(".norm1." in n or ".norm2." in n for n in gnames)
        for k, v in model.state_dict().items():          # running statistics after ONE training forward
            if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
                out["bn/" + k] = v.float().numpy() if v.is_floating_point() else v.numpy()
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
        print(name, "M' =", len(d["b_ids"]), "M =", len(d["mconf"]), "draws", [tuple(x.shape) for x in draws], "grads", len(gnames))


if __name__ == "__main__":
    torch.set_num_threads(GOLDEN_CPU_THREADS)
    only = [a for a in sys.argv[1:] if not a.startswith("--")]
    steps = {"contract": gen_contract, "e2e": gen_e2e, "batch": gen_batch, "train": gen_train}
    for k, fn in steps.items():
        if not only or k in only:
            fn()
