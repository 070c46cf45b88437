"""CPU-side checks of the non-finite step guard: its C entry points, the host table of Adam bias corrections, and the parameter
mapping of tasks.Trainer (skip_nonfinite defaults to use_amp, as the reference's GradScaler exists exactly under use_amp)."""
import ctypes
import ctypes.util

import numpy as np
import pytest

from mmdti_hip import _abi

NEW = ("mmdti_sumsq_check_f32", "mmdti_adam_step_guarded", "mmdti_adam_bias_table")


def test_guard_entry_points_are_declared_and_exported():
    protos = _abi.parse_header()
    dll = ctypes.CDLL(_abi.LIB_PATH)
    for name in NEW:
        assert name in protos and hasattr(dll, name), name
    assert protos["mmdti_adam_step_guarded"][2][-1] == "guard"
    assert dll.mmdti_abi_version() == _abi.header_constants()["MMDTI_ABI_VERSION"]


def test_bias_table_is_the_host_powf_of_every_step():
    lib = _abi.lib()
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.powf.restype, libm.powf.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
    steps = 300
    tab = np.full(2 * steps, -1.0, dtype=np.float32)
    lib.mmdti_adam_bias_table(0.9, 0.999, steps, tab.ctypes.data)
    for t in range(1, steps + 1):
        bc1 = np.float32(1.0) - np.float32(libm.powf(0.9, float(t)))
        bc2 = np.sqrt(np.float32(1.0) - np.float32(libm.powf(0.999, float(t))))
        assert tab[2 * t - 2] == bc1 and tab[2 * t - 1] == bc2, t
    with pytest.raises(_abi.MMDTIError):
        lib.mmdti_adam_bias_table(0.9, 0.999, 0, tab.ctypes.data)


@pytest.mark.parametrize("params,expect", [(dict(use_amp=True), True), (dict(use_amp=False), False), (dict(), False),
                                           (dict(use_amp=True, skip_nonfinite=False), False),
                                           (dict(use_amp=False, skip_nonfinite=True), True)])
def test_trainer_guards_exactly_where_the_reference_has_a_scaler(params, expect):
    from mmdti_hip.tasks import Trainer
    tr = Trainer(task="regression", metrics="mse", **params)
    assert tr.skip_nonfinite is expect
