"""One-call swap of the MI355X-native module into a checkout of the reference.

    import onepose_plus_plus_amd.dropin as dropin
    dropin.install()                      # before (or after) the reference's own imports
    from src.inference.inference_OnePosePlus import build_model      # now builds the HIP module

`install()` makes both import paths the reference uses resolve to `onepose_plus_plus_amd.OnePosePlus_model`:
  * `from src.models.OnePosePlus.OnePosePlusModel import OnePosePlus_model`
        (src/inference/inference_OnePosePlus.py:11, demo.py:17)
  * `from src.models.OnePosePlus import OnePosePlus_model`
        (src/lightning_model/OnePosePlus_lightning_model.py:8 via src/models/OnePosePlus/__init__.py:1)
and, with `pnp=True` (or `pnp="epnp"` / `"loransac"` / `"auto"`), routes `src.utils.metric_utils.ransac_PnP` (called by `compute_query_pose_errors`,
metric_utils.py:262-270, i.e. by every caller of the matcher: inference worker, demo, validation step) to the
on-device `onepose_plus_plus_amd.pose.ransac_PnP`, which keeps the reference's signature and return tuple (`pnp="epnp"`:
with `solver="epnp"`, the reference's own minimal solver and adaptive stop; `pnp="loransac"`: LO-RANSAC with robust
refinement, the reference's pycolmap branch; `pnp="auto"`: whichever of the two the caller's `use_pycolmap_ransac` selects, as
the reference would; `pnp=True`: the default P3P solver); with `metrics=True` (off by default) `compute_query_pose_errors` itself is replaced
by a wrapper around `onepose_plus_plus_amd.metrics.compute_query_pose_errors`, which scores the poses on the device; with
`loss=True` the training step's `Loss` (src/lightning_model/losses.py) and `fine_supervision`
(src/models/OnePosePlus/utils/fine_supervision.py) resolve to `onepose_plus_plus_amd.losses`; with `optimizer=True` (off by default)
`build_optimizer` / `build_scheduler` (src/models/OnePosePlus/optimizers/optimizers.py) resolve to `onepose_plus_plus_amd.optim`.

If the reference modules were imported already their attributes are patched in place; otherwise light-weight module
objects are registered under those names, so the reference's own model files (and their kornia / timm imports) are
never loaded.  Nothing here touches the matching arithmetic: it is import plumbing only.
"""
import importlib
import sys
import types

from .model import OnePosePlus_model

_MODEL_PATHS = ("src.models.OnePosePlus.OnePosePlusModel", "src.models.OnePosePlus")
_METRICS_CALLERS = ("src.inference.inference_OnePosePlus_worker", "src.lightning_model.OnePosePlus_lightning_model")


def _real_dirs(name):
    """directories of package `name` found on sys.path (empty on a box without the reference checkout)"""
    import os
    rel = os.path.join(*name.split("."))
    return [os.path.join(p, rel) for p in sys.path if p and os.path.isdir(os.path.join(p, rel))]


def _ensure_package(name):
    """registers empty parent packages (src, src.models) only when the real ones cannot be imported"""
    if name in sys.modules:
        return sys.modules[name]
    try:
        return importlib.import_module(name)
    except Exception:
        mod = types.ModuleType(name)
        mod.__path__ = _real_dirs(name)       # sub-modules that do import cleanly still come from the checkout
        sys.modules[name] = mod
        parent, _, leaf = name.rpartition(".")
        if parent:
            setattr(_ensure_package(parent), leaf, mod)
        return mod


def _patch_attr(path, name, obj, done):
    """sets `path.name = obj` on the imported module, or on a light-weight stand-in registered under that path when the
    reference file was not imported yet (so that a later `from path import name` resolves to `obj`)"""
    mod = sys.modules.get(path)
    if mod is None:
        parent, _, leaf = path.rpartition(".")
        pkg = _ensure_package(parent)
        mod = types.ModuleType(path)
        sys.modules[path] = mod
        setattr(pkg, leaf, mod)
    setattr(mod, name, obj)
    done[path] = name


def _metrics_wrapper(pnp):
    """`compute_query_pose_errors(data, configs, training=False)` for the reference's callers: the model and its diameter are loaded
    as metric_utils.py:236-252 does (the reference's own `load_points_from_cad` / `model_diameter_from_bbox`), the poses come
    from `pose.ransac_PnP` (the solver `install(pnp=...)` names) -- with `pnp=False` from whatever `metric_utils.ransac_PnP` is when
    the call is made, i.e. the reference's OpenCV / pycolmap function -- and are scored on the device by `metrics.pose_metrics`"""
    import os.path as osp

    import numpy as np

    from . import metrics
    pnp_kwargs = {"solver": pnp} if isinstance(pnp, str) else {}
    if not pnp:
        def reference_pnp(*args, **kwargs):
            return sys.modules["src.utils.metric_utils"].ransac_PnP(*args, **kwargs)
        pnp_kwargs = {"ransac_PnP": reference_pnp}

    def compute_query_pose_errors(data, configs, training=False):
        model_vertices = diameter = None
        if "eval_ADD_metric" in configs and configs["eval_ADD_metric"] and not training:
            from src.utils.sample_points_on_cad import load_points_from_cad, model_diameter_from_bbox
            image_path = data["query_image_path"]
            root = image_path.rsplit("/", 3)[0]
            model_path = osp.join(root, "model_eval.ply")
            if not osp.exists(model_path):
                model_path = osp.join(root, "model.ply")
            diameter_file_path = osp.join(root, "diameter.txt")
            if osp.exists(model_path):       # upstream logs an error and evaluates no ADD otherwise
                model_vertices, bbox = load_points_from_cad(model_path)   # N*3
                diameter = np.loadtxt(diameter_file_path) if osp.exists(diameter_file_path) else model_diameter_from_bbox(bbox)
        return metrics.compute_query_pose_errors(data, configs, training=training, model_vertices=model_vertices, diameter=diameter,
                                                 **pnp_kwargs)

    return compute_query_pose_errors


def install(pnp=True, loss=True, metrics=False, optimizer=False):
    """-> dict of what was patched (for logging / tests).  pnp: True (P3P solver), "epnp" (the reference's EPnP), "loransac" (its
    pycolmap branch), "auto" (the one of the two that the caller's `use_pycolmap_ransac` selects) or False.  metrics: True also
    replaces `src.utils.metric_utils.compute_query_pose_errors` by the on-device scoring of `onepose_plus_plus_amd.metrics`
    (recorded under "src.utils.metric_utils:compute_query_pose_errors") and rebinds the name in the reference's two callers when
    they were imported already (recorded under "<module>:compute_query_pose_errors"); off by default.  With `pnp=False` the
    wrapper scores the poses of the reference's own `ransac_PnP` (OpenCV / pycolmap) on the device.  optimizer: True makes
    `src.models.OnePosePlus.optimizers.optimizers` a stand-in that holds `onepose_plus_plus_amd.optim.build_optimizer` /
    `build_scheduler` (`configure_optimizers`, OnePosePlus_lightning_model.py:162-165, then returns a `FusedAdam`) and rebinds
    the two names in the Lightning module when it was imported already; off by default"""
    done = {}
    for path in _MODEL_PATHS:
        mod = sys.modules.get(path)
        if mod is None:
            parent, _, leaf = path.rpartition(".")
            pkg = _ensure_package(parent)
            mod = types.ModuleType(path)
            if path == "src.models.OnePosePlus":
                # a stand-in for the package (its real __init__ would load the reference model and kornia / timm); the
                # reference's other sub-packages (optimizers, utils, ...) stay importable from the checkout, if there is one
                mod.__path__ = _real_dirs(path)
            sys.modules[path] = mod
            setattr(pkg, leaf, mod)
        mod.OnePosePlus_model = OnePosePlus_model
        done[path] = "OnePosePlus_model"
    # keep the sub-module reachable as an attribute of the package (import machinery convention)
    setattr(sys.modules["src.models.OnePosePlus"], "OnePosePlusModel", sys.modules["src.models.OnePosePlus.OnePosePlusModel"])
    if pnp not in (False, None, True, "epnp", "loransac", "auto"):
        raise ValueError("pnp must be True, False, 'epnp', 'loransac' or 'auto', got %r" % (pnp,))
    if pnp:
        from .pose import ransac_PnP
        if isinstance(pnp, str):
            import functools
            ransac_PnP = functools.partial(ransac_PnP, solver=pnp)
        try:
            mu = importlib.import_module("src.utils.metric_utils")
            mu.ransac_PnP = ransac_PnP
            done["src.utils.metric_utils"] = "ransac_PnP (%s)" % pnp if isinstance(pnp, str) else "ransac_PnP"
        except Exception as e:      # the reference (or one of its dependencies) is not importable here
            done["src.utils.metric_utils"] = "not patched: %s" % (e,)
    if metrics:
        key = "src.utils.metric_utils:compute_query_pose_errors"
        try:
            mu = importlib.import_module("src.utils.metric_utils")
            mu.compute_query_pose_errors = _metrics_wrapper(pnp)
            wrapper = mu.compute_query_pose_errors
            done[key] = "compute_query_pose_errors (%s)" % pnp if isinstance(pnp, str) else "compute_query_pose_errors"
            # the reference's callers bind the name when they are imported (inference_OnePosePlus_worker.py:4,
            # OnePosePlus_lightning_model.py:15): one imported before install() is rebound as well
            for path in _METRICS_CALLERS:
                caller = sys.modules.get(path)
                if caller is not None and hasattr(caller, "compute_query_pose_errors"):
                    caller.compute_query_pose_errors = wrapper
                    done[path + ":compute_query_pose_errors"] = done[key]
        except Exception as e:      # the reference (or one of its dependencies) is not importable here
            done[key] = "not patched: %s" % (e,)
    if loss:
        # training step (src/lightning_model/OnePosePlus_lightning_model.py:9,14): `fine_supervision(batch, hparams)` and
        # `Loss(hparams["loss"])` -> the module's own (the focal loss over the B x N x L matrix runs in libopp_hip.so)
        from .losses import Loss, fine_supervision
        _patch_attr("src.lightning_model.losses", "Loss", Loss, done)
        _patch_attr("src.models.OnePosePlus.utils.fine_supervision", "fine_supervision", fine_supervision, done)
        lm = sys.modules.get("src.lightning_model.OnePosePlus_lightning_model")
        if lm is not None:          # imported before install(): its module-level names were bound already
            lm.Loss, lm.fine_supervision = Loss, fine_supervision
            done["src.lightning_model.OnePosePlus_lightning_model"] = "Loss, fine_supervision"
    if optimizer:
        from .optim import build_optimizer, build_scheduler
        path = "src.models.OnePosePlus.optimizers.optimizers"
        standin = types.ModuleType(path)                 # replaces the reference's file even when it was imported already
        standin.build_optimizer, standin.build_scheduler = build_optimizer, build_scheduler
        parent = "src.models.OnePosePlus.optimizers"
        pkg = sys.modules.get(parent)
        if pkg is None:
            pkg = types.ModuleType(parent)
            pkg.__path__ = _real_dirs(parent)
            sys.modules[parent] = pkg
            setattr(sys.modules["src.models.OnePosePlus"], "optimizers", pkg)
        sys.modules[path] = standin
        pkg.optimizers = standin
        done[path] = "build_optimizer, build_scheduler"
        lm = sys.modules.get("src.lightning_model.OnePosePlus_lightning_model")
        if lm is not None:          # imported before install(): OnePosePlus_lightning_model.py:10-13 bound the names already
            lm.build_optimizer, lm.build_scheduler = build_optimizer, build_scheduler
            done["src.lightning_model.OnePosePlus_lightning_model:build_optimizer"] = "build_optimizer, build_scheduler"
    return done
