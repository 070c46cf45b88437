"""Fused attention for 257-512 tokens, host side: the C ABI declares the long entry points and the eligibility rule covers them."""
import pytest

from mmdti_hip import _abi


def test_header_declares_long_attention_with_the_short_argument_lists():
    protos = _abi.parse_header()
    for long_name, short_name in (("mmdti_attn_long_fwd", "mmdti_attn_fwd"), ("mmdti_attn_long_bwd", "mmdti_attn_bwd")):
        assert long_name in protos, long_name
        assert protos[long_name][0] is protos[short_name][0]
        assert protos[long_name][1] == protos[short_name][1]          # same argument types, same order
        assert protos[long_name][2] == protos[short_name][2]          # ... and names


def test_library_exports_long_attention_and_abi_version_is_the_headers():
    lib = _abi.lib()                                                   # raises if a declared symbol is not exported
    assert "mmdti_attn_long_fwd" in lib.protos and "mmdti_attn_long_bwd" in lib.protos
    assert lib._dll.mmdti_abi_version() == lib.const["MMDTI_ABI_VERSION"]


def test_attn_eligible_up_to_512():
    from mmdti_hip import ops
    assert ops.attn_eligible(512, 512, 64, 512)
    assert ops.attn_eligible(258, 300, 32, 512)
    assert ops.attn_eligible(300, 258, 32, 512)
    assert ops.attn_eligible(256, 256, 64, 512) and ops.attn_eligible(1, 1, 16, 64)
    assert not ops.attn_eligible(513, 16, 64, 512)
    assert not ops.attn_eligible(16, 513, 64, 512)
    assert not ops.attn_eligible(128, 128, 48, 96)                     # head_dim 48
    old = ops.FUSED_ATTN
    ops.FUSED_ATTN = False
    try:
        for shape in ((512, 512, 64, 512), (258, 300, 32, 512), (16, 16, 64, 512)):
            assert not ops.attn_eligible(*shape)
    finally:
        ops.FUSED_ATTN = old


def test_one_dispatch_point_picks_the_pair():
    from mmdti_hip import ops
    assert ops.attn_dispatch(256, 256) == (ops.attn_fwd, ops.attn_bwd)
    assert ops.attn_dispatch(130, 160) == (ops.attn_fwd, ops.attn_bwd)
    for Lq, Lk in ((257, 16), (16, 257), (258, 384), (512, 512)):
        assert ops.attn_dispatch(Lq, Lk) == (ops.attn_long_fwd, ops.attn_long_bwd)


def test_longer_than_512_warns_once(monkeypatch):
    from mmdti_hip import ops
    monkeypatch.setattr(ops, "_warned_long", False)
    with pytest.warns(RuntimeWarning, match="512"):
        ops.warn_unfused_length(600, 130)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ops.warn_unfused_length(600, 130)                              # second time: silent
        ops.warn_unfused_length(512, 512)


def test_long_attention_instantiations_use_no_scratch():
    """The 24- / 32-tile instantiations hold their score rows in registers and address LDS images past 64 KiB through hidden second
    bases (attn.hip, attn_far_rows): that they need no scratch depends on the compiler's register allocation, so a toolchain that
    reintroduces it fails here.  Device-only compile of attn.hip with the resource-usage remarks of the build's flags."""
    import os, re, shutil, subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    assert hipcc, "hipcc not found: the build needs it too"
    src = os.path.join(_abi.REPO_ROOT, "mm-dti_amd", "csrc", "attn.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]
    seen = 0
    for b in blocks:
        name = b.split()[0]
        m = re.search(r"attn_(fwd|bwd_q)_kernelILi(\d+)ELi(\d+)E", name)
        if not m or int(m.group(3)) <= 16:
            continue
        seen += 1
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        assert scratch == 0, (name, scratch)
    assert seen == 12, seen                      # forward and dQ: head_dim 16 / 32 / 64 x 24 / 32 tiles
