"""CPU: `onepose_plus_plus_amd.dropin.install()` registers the HIP module under both import paths of the reference's model
(src.models.OnePosePlus.OnePosePlusModel and src.models.OnePosePlus) on a machine without the reference checkout.  The forward
itself needs a GPU: the worker's data flow is exercised on the device by tests/test_e2e_gpu.py::test_worker_flow_recovers_pose."""
import sys


def test_install_without_reference_modules_registers_both_paths():
    """On a box without the reference checkout the aliases are still importable (what the GPU tests use)."""
    from onepose_plus_plus_amd import OnePosePlus_model, dropin
    saved = {k: v for k, v in sys.modules.items() if k == "src" or k.startswith("src.")}
    saved_path = list(sys.path)
    try:
        for k in saved:
            sys.modules.pop(k, None)
        dropin.install(pnp=False)
        from src.models.OnePosePlus.OnePosePlusModel import OnePosePlus_model as A
        from src.models.OnePosePlus import OnePosePlus_model as B
        assert A is OnePosePlus_model and B is OnePosePlus_model
    finally:
        sys.path[:] = saved_path
        for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:     # every stand-in install() registered
            del sys.modules[k]
        sys.modules.update(saved)
