"""The deterministic mode without a GPU: workspace sizes, environment / keyword parsing, the host-side refusals (which return before any
launch), the per-stream table under a host sanitizer (a stand-alone program), and the proof that the default mode touches nothing."""
import ctypes
import os
import shutil
import subprocess
import sys

import pytest

from mmdti_hip import _abi, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x10000            # fake, 16-byte aligned device address: nothing here dereferences it


@pytest.fixture
def mode_on():
    lib = _abi.lib()
    lib.mmdti_set_deterministic(1)
    yield lib
    lib.mmdti_set_deterministic(0)
    for s in (0, 0x40, 0x80):
        lib.mmdti_det_workspace(s, 0, 0)


# ------------------------------------------------------------------------------------------------ sizes
def test_workspace_bytes_against_hand_computed_sizes():
    # LayerNorm backward: [workgroups][3][D] fp32; rows per wave = max(4, ceil(rows / (4 waves * (3 or 2 workgroups per CU) * 256 CUs)))
    assert ops.det_workspace_bytes("layernorm_bwd", 37, 512) == 3 * 3 * 512 * 4                # ceil(37 / 16) = 3 workgroups
    assert ops.det_workspace_bytes("layernorm_bwd", 12805, 512) == 641 * 3 * 512 * 4           # 5 rows per wave: ceil(12805 / 20)
    assert ops.det_workspace_bytes("layernorm_bwd", 12805, 1024) == 458 * 3 * 1024 * 4         # 7 rows per wave: ceil(12805 / 28)
    assert ops.det_workspace_bytes("layernorm_bwd", 37, 1024) == 3 * 3 * 1024 * 4
    # column sums: [row groups][cols] fp32, a row group per 64 rows, at most 1024
    assert ops.det_workspace_bytes("colsum", 1000, 512) == 16 * 512 * 4
    assert ops.det_workspace_bytes("colsum", 4160, 256) == 65 * 256 * 4                          # the bias gradient of dw [256, 256] over 4160 rows
    assert ops.det_workspace_bytes("colsum", 333, 50) == 6 * 50 * 4
    assert ops.det_workspace_bytes("colsum", 318, 512) == 5 * 512 * 4                            # V == 1 embedding gradient
    assert ops.det_workspace_bytes("colsum", 10 ** 6, 512) == 1024 * 512 * 4
    # one split's slab of a split-K weight gradient
    assert ops.det_workspace_bytes("gemm_slab", 50, 512) == 50 * 512 * 4
    assert ops.det_workspace_bytes("gemm_slab", 31, 512) == 31 * 512 * 4
    with pytest.raises(_abi.MMDTIError, match="unknown site"):
        _abi.lib().mmdti_det_workspace_bytes(99, 4, 4, ctypes.byref(ctypes.c_longlong()))
    with pytest.raises(_abi.MMDTIError, match="bad shape"):
        _abi.lib().mmdti_det_workspace_bytes(1, 16, 4096, ctypes.byref(ctypes.c_longlong()))    # LayerNorm rows end at 2048 columns
    # the default per-stream workspace covers every site of the shapes above, and the widest LayerNorm row the kernels take
    cap = ops.det_workspace_mb({}) << 20
    assert cap >= ops.det_workspace_bytes("layernorm_bwd", 10 ** 6, 2048) and cap >= ops.det_workspace_bytes("colsum", 10 ** 6, 4096)


def test_new_symbols_are_in_the_header_and_nothing_else_changed_its_arguments():
    protos = _abi.parse_header()
    assert protos["mmdti_set_deterministic"][2] == ["on"]
    assert protos["mmdti_det_workspace"][2] == ["stream", "ws", "bytes"]
    assert protos["mmdti_det_workspace_bytes"][2] == ["site", "rows", "cols", "bytes_out"]
    assert protos["mmdti_layernorm_bwd"][2][-1] == "dx_colsum" and len(protos["mmdti_layernorm_bwd"][2]) == 22
    assert protos["mmdti_colsum_bf16"][2] == ["stream", "x_bf16", "rows", "cols", "ld", "out"]


# ------------------------------------------------------------------------------------------------ switches
def test_environment_and_keyword_parsing():
    for v in ("1", "true", "on", "yes", "2", " 1 "):
        assert ops.deterministic_default({"MMDTI_DETERMINISTIC": v}) is True, v
    for v in ("", "0", "false", "FALSE", "off", "no", " 0 "):
        assert ops.deterministic_default({"MMDTI_DETERMINISTIC": v}) is False, v
    assert ops.deterministic_default({}) is False
    assert ops.det_workspace_mb({}) == 32 and ops.det_workspace_mb({"MMDTI_DET_WORKSPACE_MB": "8"}) == 8
    with pytest.raises(_abi.MMDTIError):
        ops.det_workspace_mb({"MMDTI_DET_WORKSPACE_MB": "0"})
    import inspect
    from mmdti_hip.trainer import FineTuner
    from mmdti_hip.tasks.trainer import Trainer
    assert inspect.signature(FineTuner.__init__).parameters["deterministic"].default is None
    assert Trainer(task="regression", metrics="mse", deterministic=True).deterministic is True
    assert Trainer(task="regression", metrics="mse").deterministic is None


def test_the_environment_default_enters_the_mode_lazily():
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from mmdti_hip import ops, _abi\n"
            "assert ops._stream is ops._stream_boot and not ops.is_deterministic() and _abi._lib is None\n"
            "print('lazy')\n") % (ROOT, os.path.join(ROOT, "mm-dti_amd"))
    for env_val, want in (("1", "lazy"), ("0", None)):
        env = dict(os.environ, MMDTI_DETERMINISTIC=env_val)
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
        if want:
            assert r.returncode == 0 and r.stdout.strip() == want, r.stderr[-400:]
        else:
            assert r.returncode != 0 and "AssertionError" in r.stderr


# ------------------------------------------------------------------------------------------------ refusals, before any launch
def _ln_bwd(lib, stream, dgamma=PTR):
    return lib.mmdti_layernorm_bwd(stream, PTR, 1, 0, PTR, PTR, PTR, PTR, 37, 512, 0, PTR, dgamma, dgamma, 0, 0.0, 0, 0, 0, 0.0, 0, 0)


def test_sites_refuse_a_stream_without_a_workspace(mode_on):
    lib = mode_on
    with pytest.raises(_abi.MMDTIError, match=r"layernorm_bwd: deterministic mode is on and stream .* has no reduction workspace"):
        _ln_bwd(lib, 0x40)
    with pytest.raises(_abi.MMDTIError, match=r"colsum_bf16: deterministic mode is on and stream"):
        lib.mmdti_colsum_bf16(0x40, PTR, 1000, 512, 512, PTR)
    # too small: LayerNorm backward over 37 x 512 needs 3 * 3 * 512 * 4 = 18432 bytes
    lib.mmdti_det_workspace(0x40, PTR, 18431)
    with pytest.raises(_abi.MMDTIError, match=r"layernorm_bwd: deterministic mode: the workspace of stream .* holds 18431 bytes, 18432 needed"):
        _ln_bwd(lib, 0x40)
    # another stream's workspace does not count
    lib.mmdti_det_workspace(0x80, PTR, 1 << 20)
    with pytest.raises(_abi.MMDTIError, match="18431 bytes"):
        _ln_bwd(lib, 0x40)
    # a weight gradient that carries its bias gradient: the column-sum pass needs the workspace (dw [256, 256] over 4160 rows, db given)
    from gemm_plan_helpers import case, gemm_call_args
    args = gemm_call_args(case(256, 256, 4160, tA=1, tB=1, sk=8, out="atomic", arowsum=1))
    with pytest.raises(_abi.MMDTIError, match=r"gemm \(arowsum bias gradient\): deterministic mode is on and stream .* no reduction workspace of 66560 bytes"):
        lib.mmdti_gemm_bf16(0x40, *args)
    with pytest.raises(_abi.MMDTIError, match="workspace needs bytes > 0 and 16-byte alignment"):
        lib.mmdti_det_workspace(0x40, PTR + 8, 64)


def test_sites_without_a_fixed_order_form_refuse_in_the_mode(mode_on):
    lib = mode_on
    with pytest.raises(_abi.MMDTIError, match="sumsq_f32: deterministic mode needs the ws form"):
        lib.mmdti_sumsq_f32(0, PTR, 1024, PTR, 0, 0)
    with pytest.raises(_abi.MMDTIError, match="ct_loss_fwd: deterministic mode needs row_ws"):
        lib.mmdti_ct_loss_fwd(0, 0, PTR, 8, 64, PTR, 0, 0, PTR, 0, 1.0, 0.5, 0.1, 1.0, PTR, PTR, 0)
    # the fused per-pair half of the round-1 pair-bias chain (MMDTI_GBF_FULL_BWD=0) has no fixed-order form
    with pytest.raises(_abi.MMDTIError, match="gbf_bias_bwd .*refused in the deterministic mode"):
        lib.mmdti_gbf_bias_bwd(0, PTR, PTR, PTR, 8, PTR, PTR, PTR, PTR, PTR, PTR, PTR, 3, 40, 40, 128, 128, 64, 16, 1, PTR, PTR, PTR, PTR, PTR, PTR)
    # the unfused feature backward has one, and needs its stream's workspace: 100 pairs -> 7 workgroups x (2 E + 2 K) floats
    with pytest.raises(_abi.MMDTIError, match="gbf_features_bwd: deterministic mode is on and stream"):
        lib.mmdti_gbf_features_bwd(0x40, PTR, PTR, PTR, PTR, PTR, PTR, 100, 128, 16, PTR, PTR, PTR, PTR, PTR)
    assert ops.det_workspace_bytes("gbf_features_bwd", 100, 2 * 16 + 2 * 128) == 7 * 288 * 4
    # the fused pair-bias backward without its slabs (MMDTI_GBF_SLABS=0) would meet in atomics
    with pytest.raises(_abi.MMDTIError, match="gbf_bias_bwd_full: deterministic mode needs the workspace"):
        lib.mmdti_gbf_bias_bwd_full(0, PTR, PTR, PTR, 8, PTR, PTR, PTR, PTR, PTR, PTR, PTR, 3, 40, 40, 128, 128, 64, 16, 1, PTR, PTR, PTR, PTR, PTR, PTR,
                                    PTR, PTR, 0, 0, 0, 0)


# ------------------------------------------------------------------------------------------------ the table under a sanitizer
def test_stream_table_and_split_rule_under_address_and_undefined_sanitizers(tmp_path):
    """tests/det_table_main.cpp: a stand-alone program over csrc/det.h (registration, replacement, concurrent use, the workspace sizes and
    the rule that lowers a split count to what fits), built with -fsanitize=address,undefined.  Nothing loaded into Python is sanitized."""
    cxx = os.environ.get("HIPCC") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc"))
    assert cxx, "no hipcc (the compiler the library itself is built with)"
    exe = str(tmp_path / "det_table_main")
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "det_table_main.cpp"), "-o", exe, "-lpthread"], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout[-600:], r.stderr[-600:])


# ------------------------------------------------------------------------------------------------ the default mode is not touched
class _Stub:
    def __init__(self):
        self.calls = []
        self.const = {"MMDTI_DET_LAYERNORM_BWD": 1}

    def __getattr__(self, name):
        if name.startswith("mmdti_"):
            return lambda *a: self.calls.append((name,) + a)
        raise AttributeError(name)


class _FakeTensor:
    def data_ptr(self):
        return 0x7000

    def numel(self):
        return 32 << 20


def test_default_mode_never_touches_the_switch_or_the_table(monkeypatch):
    stub = _Stub()
    monkeypatch.setattr(ops, "lib", lambda: stub)
    monkeypatch.setattr(ops, "_raw_device", lambda: 0)
    handles = iter([0, 0, 0x40, 0, 0x40, 0x80, 0x80])
    monkeypatch.setattr(ops, "_raw_stream", lambda dev: next(handles))
    monkeypatch.setattr(ops.torch, "empty", lambda *a, **k: _FakeTensor())
    monkeypatch.setattr(ops.torch.cuda, "is_available", lambda: False)
    assert not ops.is_deterministic() and ops._stream is ops._stream_fast
    # off: launches take their stream, side streams pass through det_register, the switch is set to what it already is -- no call
    assert ops._stream() == 0 and ops.det_register(0x40) == 0x40
    ops.set_deterministic(False)
    assert stub.calls == []
    try:
        # on: the flag once, then one workspace per stream at its first use
        ops.set_deterministic(True)
        ops.set_deterministic(True)
        assert stub.calls == [("mmdti_set_deterministic", 1)]
        assert [ops._stream() for _ in range(4)] == [0, 0x40, 0, 0x40]
        assert ops.det_register(0x80) == 0x80 and ops._stream() == 0x80
        assert stub.calls[1:] == [("mmdti_det_workspace", h, 0x7000, 32 << 20) for h in (0, 0x40, 0x80)]
    finally:
        ops.set_deterministic(False)
    # off again: every stream forgotten, the flag cleared, the fast _stream back
    assert sorted(stub.calls[4:7]) == [("mmdti_det_workspace", h, 0, 0) for h in (0, 0x40, 0x80)]
    assert stub.calls[7:] == [("mmdti_set_deterministic", 0)]
    assert ops._stream is ops._stream_fast and not ops._det_ws and not ops.is_deterministic()
