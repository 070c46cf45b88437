"""The adapted sequencers (include/mmdti_hip.h "Sequenced layers that carry LoRA adapters"; csrc/layers.hip), host side, no GPU: the
twelve symbols and the two tagged blocks, the launch-free layout queries against an independent statement of their byte counts, what
every call refuses before its first launch, and the decisions of paths.py with adapter_seq."""
import ctypes
import os
import shutil
import subprocess

import pytest

from mmdti_hip import _abi, paths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x10000            # fake, 16-byte aligned device address: nothing here dereferences it
CALLS = ("mmdti_unimol_lora_layer_fwd", "mmdti_unimol_lora_layer_bwd", "mmdti_unimol_lora_stack_fwd", "mmdti_unimol_lora_stack_bwd",
         "mmdti_bert_lora_layer_fwd", "mmdti_bert_lora_cross_layer_fwd", "mmdti_bert_lora_layer_bwd", "mmdti_bert_lora_cross_layer_bwd",
         "mmdti_bert_lora_stack_fwd", "mmdti_bert_lora_stack_bwd")
QUERIES = ("mmdti_unimol_lora_stack_layout", "mmdti_bert_lora_stack_layout")
BLOCKS = ("mmdti_lora_adapter_t", "mmdti_bert_split_t")
NL = 2


def test_symbols_are_in_the_header_the_library_and_the_documents():
    protos = _abi.parse_header()
    assert set(CALLS + QUERIES) <= set(protos)
    dll = ctypes.CDLL(_abi.LIB_PATH)
    assert all(hasattr(dll, n) for n in CALLS + QUERIES)
    assert _abi.header_constants()["MMDTI_ABI_VERSION"] == 2 == dll.mmdti_abi_version()          # purely additive
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert f"exporting exactly the {len(protos)} symbols" in doc and all(n in doc for n in CALLS + QUERIES)


def test_the_binding_builds_the_two_blocks_from_the_header_alone(tmp_path):
    structs = _abi.parse_structs(tagged=True)
    assert set(BLOCKS) <= set(structs) and set(structs) - set(BLOCKS) == set(_abi.parse_structs())
    ad = structs["mmdti_lora_adapter_t"]
    assert [f for f, _ in ad._fields_] == ["A", "B", "A_bf16", "B_bf16", "dA", "dB", "r", "scale"]
    assert [t for _, t in ad._fields_] == [ctypes.c_void_p] * 6 + [ctypes.c_int, ctypes.c_float]
    assert [f for f, _ in structs["mmdti_bert_split_t"]._fields_] == ["w_q", "w_k", "w_v", "b_q", "b_k", "b_v", "wb_q", "wb_k", "wb_v"]
    assert _abi.lib().struct("mmdti_lora_adapter_t")(r=16, scale=2.0).r == 16
    with pytest.raises(AttributeError):
        _abi.lib().struct("mmdti_lora_adapter_t")(rank=16)
    # the C compiler lays them out as ctypes does (the header compiled AS C)
    cc = os.environ.get("HIPCC") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc"))
    assert cc, "no hipcc (the compiler the library itself is built with)"
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "mmdti_hip.h"', "int main(void) {",
             '  printf("rows %lld %lld %lld\\n", MMDTI_LORA_ROW_BYTES(1), MMDTI_LORA_ROW_BYTES(4), MMDTI_LORA_ROW_BYTES(169));']
    for name in BLOCKS:
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f, _ in structs[name]._fields_]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", str(tmp_path / "layout")
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-x", "c", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120).stdout.splitlines()
    assert out[0] == "rows 256 256 11008"
    got = dict(l.split() for l in out[1:])
    want = {}
    for name in BLOCKS:
        want[name] = str(ctypes.sizeof(structs[name]))
        want.update({f"{name}.{f}": str(getattr(structs[name], f).offset) for f, _ in structs[name]._fields_})
    assert got == want and len(want) == 19


# ---- the byte counts, stated independently: the existing layouts (tests/test_layer_structs_cpu.py holds those to recorded values) plus the
# t / u rows, each room for rank 32 in bf16 and rounded up to 256 bytes like every slot of the arenas
def _up(b, to=256):
    return (b + to - 1) // to * to


def _row(rows):
    return _up(rows * 32 * 2)


def _unimol_tmp(M, D, F):
    return (M * F + 7 * M * D) * 2 + M * D * 4


def _bert_tmp(Mq, Mk, D, F, nrow):
    # dzb, da, dyb, dctx, dq [Mq,D] | du [Mq,F] | dk, dv [Mk,D] (bf16) | dz [Mq,D] fp32 | drow
    return (Mq * F + 5 * Mq * D + 2 * Mk * D) * 2 + Mq * D * 4 + _up(nrow * 4, 16)


@pytest.mark.parametrize("M, D, F, s_bytes", [(84, 64, 128, 43008), (4097, 512, 1024, 12345), (33280, 512, 2048, 1 << 20)])
def test_unimol_layout_is_the_plain_one_plus_the_rows(M, D, F, s_bytes):
    lib = _abi.lib()
    plain, out = (ctypes.c_longlong * 4)(), (ctypes.c_longlong * 5)()
    lib.mmdti_unimol_stack_layout(M, D, F, s_bytes, 0, ctypes.addressof(plain))
    lib.mmdti_unimol_lora_stack_layout(M, D, F, s_bytes, ctypes.addressof(out))
    assert out[0] == plain[0] + _row(M)                                     # one t row behind each slice
    assert out[1] == plain[1] + 2 * _row(M)                                 # one u row behind each of the two layer workspaces
    assert out[2] == _up(_unimol_tmp(M, D, F)) + _row(M) and plain[2] == _unimol_tmp(M, D, F)
    assert out[3] == 0 and out[4] == 0                                      # (three counts: nothing else is written)


@pytest.mark.parametrize("Mq, Mk, D, F, nrow", [(169, 169, 64, 128, 676), (240, 84, 512, 256, 1920), (84, 240, 64, 128, 336), (33280, 33280, 512, 2048, 266240)])
def test_bert_layout_is_the_plain_one_plus_the_rows(Mq, Mk, D, F, nrow):
    lib = _abi.lib()
    plain, out = (ctypes.c_longlong * 4)(), (ctypes.c_longlong * 5)()
    lib.mmdti_bert_stack_layout(Mq, D, F, 8 * nrow, nrow, 0, ctypes.addressof(plain))
    lib.mmdti_bert_lora_stack_layout(Mq, Mk, D, F, 8 * nrow, nrow, ctypes.addressof(out))
    assert out[0] == plain[0] + 3 * _row(Mq)
    assert out[1] == plain[1] + 3 * _row(Mq)
    assert out[2] == _up(_bert_tmp(Mq, Mq, D, F, nrow)) + 3 * _row(Mq) and _bert_tmp(Mq, Mq, D, F, nrow) == plain[2]
    assert out[3] == _up(_bert_tmp(Mq, Mk, D, F, nrow)) + 3 * _row(max(Mq, Mk))
    assert out[4] == 3 * _row(max(Mq, Mk))
    with pytest.raises(_abi.MMDTIError, match="bad arguments"):
        lib.mmdti_bert_lora_stack_layout(Mq, 0, D, F, 8 * nrow, nrow, ctypes.addressof(out))
    with pytest.raises(_abi.MMDTIError, match="bad arguments"):
        lib.mmdti_unimol_lora_stack_layout(Mq, D, F, 0, 0)


# ---- what every call refuses before its first launch ------------------------------------------------------------------------------------
UNI_RUN = dict(seed=1, M=128, B=2, N=64, H=32, D=256, F=256, ld=64, pair_layout=3, act_fwd=4, act_dx=5, ln_max_k=0, fwd_f16=0, scale=0.35, p_res=0.0,
               p_att=0.0)
BERT_RUN = dict(seed=1, Mq=128, Mk=128, B=2, Lq=64, Lk=64, heads=4, D=256, F=256, q_rows=0, act_fwd=4, act_dx=5, ln_max_k=0, fwd_f16=0, scale=0.125,
                p_hid=0.0, p_att=0.0, eps=1e-12)


def _full(cls, **over):
    """a block whose every pointer field holds a dummy address"""
    return cls(**dict({f: PTR for f, t in cls._fields_ if t is ctypes.c_void_p}, **over))


def _call(name, rank=8, small=False, null=None):
    """Call `name` with complete blocks of dummy addresses; rank: of the LAST adapter block; small: every byte count 16; null: the
    argument to pass as 0."""
    lib = _abi.lib()
    tower = "unimol" if "unimol" in name else "bert"
    stack = "_stack_" in name
    n_ad = (NL if stack else 1) * (1 if tower == "unimol" else 3)
    AD = lib.struct("mmdti_lora_adapter_t")
    run = lib.struct(f"mmdti_{tower}_run_t")(**(UNI_RUN if tower == "unimol" else BERT_RUN))
    P, S, SP = lib.struct(f"mmdti_{tower}_layer_t"), lib.struct(f"mmdti_{tower}_saved_t"), lib.struct("mmdti_bert_split_t")
    keep = dict(run_block=run, layer=_full(P), layers=(P * NL)(*[_full(P) for _ in range(NL)]), saved=_full(S),
                split=(SP * NL)(*[_full(SP) for _ in range(NL)]),
                lora=(AD * n_ad)(*[_full(AD, r=(rank if j == n_ad - 1 else 8), scale=2.0) for j in range(n_ad)]))
    args = []
    for argname, t in zip(lib.protos[name][2], lib.protos[name][1]):
        if argname == null:
            args.append(0)
        elif argname in keep:
            args.append(ctypes.addressof(keep[argname]))
        elif t is ctypes.c_void_p:
            args.append(PTR)
        elif t is ctypes.c_longlong:             # (s_bytes / stats_bytes: a layer's logits / statistics; else the bytes of an arena or workspace)
            args.append(4096 if argname in ("s_bytes", "stats_bytes") else 16 if small else 1 << 40)
        elif t is ctypes.c_float:
            args.append(1e-5)
        else:
            args.append({"nl": NL, "next_mode": 1}.get(argname, 1))
    getattr(lib, name)(*args)


@pytest.mark.parametrize("name", CALLS)
def test_refused_before_any_launch(name):
    """(a complete call is never made: it would launch)"""
    names = _abi.lib().protos[name][2]
    assert names[1] == "run_block" and "lora" in names
    for null in ("run_block", "layers" if "layers" in names else "layer", "split" if "split" in names else "run_block",
                 "saved" if "saved" in names else "run_block"):
        with pytest.raises(_abi.MMDTIError, match="null (block|argument)"):
            _call(name, null=null)
    if "_stack_" in name:                       # a stack call takes every layer's blocks: no adapter array, no call
        with pytest.raises(_abi.MMDTIError, match="null (block|argument|adapter blocks)"):
            _call(name, null="lora")
    for rank in (4, 12, 64, -8):
        with pytest.raises(_abi.MMDTIError, match=rf"rank 8, 16 or 32 \(got {rank}\)"):
            _call(name, rank=rank)
    if "t" in names:                            # an adapter's t row
        with pytest.raises(_abi.MMDTIError, match="needs its t"):
            _call(name, null="t")
    sized = [n for n in names if n in ("arena_bytes", "ws_bytes")]
    assert bool(sized) == (not name.endswith("layer_fwd"))
    if sized:
        with pytest.raises(_abi.MMDTIError, match="too small"):
            _call(name, small=True)


def test_the_existing_calls_refuse_what_they_refused():
    """the bodies are shared: the plain entry points still insist on the weight-gradient buffers and on dx_out"""
    lib = _abi.lib()
    run = lib.struct("mmdti_unimol_run_t")(**UNI_RUN)
    P, S = lib.struct("mmdti_unimol_layer_t"), lib.struct("mmdti_unimol_saved_t")
    big = 1 << 40
    for layer, dx_out in ((_full(P, dw_in=0), PTR), (_full(P), 0)):
        with pytest.raises(_abi.MMDTIError, match="null argument"):
            lib.mmdti_unimol_layer_bwd(0, ctypes.addressof(run), ctypes.addressof(layer), ctypes.addressof(_full(S)), 1, 1, 1, PTR, PTR, dx_out, PTR, PTR, PTR, 1,
                                       PTR, big)


# ---- paths ----------------------------------------------------------------------------------------------------------------------------------
SW = paths.Switches(layer_seq=True, stack_seq=True, stack_max_rows=8192, grouped_dw=True, grouped_dw_min_rows=0, fwd_f16=True, timer=False)


def test_adapter_seq_ok_wants_a_frozen_base_and_training_adapters():
    ok = paths.adapter_seq_ok
    assert ok(True, [False] * 12, [True, True])
    assert not ok(False, [False] * 12, [True, True])                        # MMDTI_LORA_SEQ=0
    assert not ok(True, [False] * 11 + [True], [True, True])                # a trainable base parameter
    assert not ok(True, [False] * 12, [True, False])                        # a frozen adapter
    assert not ok(True, [False] * 12, [])                                   # no adapter at all
    assert not ok(True, [False] * 12, [True, True], fused_attn=False)


def test_adapted_layers_take_the_sequencers_with_adapter_seq():
    kw = dict(adapters=True, adapter_seq=True)
    assert paths.unimol_layer_fwd(SW, True, True, 512, 64, **kw) == paths.LAYER
    assert paths.unimol_tower_fwd(SW, paths.LAYER, True, 15, 4096, False, True, **kw) == paths.STACK
    assert paths.unimol_tower_fwd(SW, paths.LAYER, True, 15, 8192, False, True, **kw) == paths.LAYER     # above the stack's rows
    # no grouped weight gradient: widths that are no multiple of 256 and a layer none of whose parameters "trains in full"
    assert paths.unimol_tower_bwd(SW, True, 2, 0, True, True, 64, 128, 84, [False, False], adapter_seq=True) == paths.LAYER
    assert paths.unimol_tower_bwd(SW, True, 2, 0, True, True, 64, 128, 84, [False, False]) == paths.OPS
    assert paths.unimol_layer_bwd(paths.LAYER, True, False, False, **kw) == paths.LAYER
    assert paths.unimol_layer_bwd(paths.LAYER, True, True, False, **kw) == paths.LAYER                    # (nothing to hold back)
    assert paths.unimol_layer_bwd(paths.LAYER, False, False, False, **kw) == paths.OPS                    # no bf16 copy from above
    assert paths.bert_tower_fwd(SW, True, True, 6, 4096, **kw) == paths.STACK
    for self_attn in (True, False):
        for fused_proj in (True, False):                                                                   # (does not apply)
            assert paths.bert_layer_fwd(SW, self_attn, fused_proj, True, 64, 128, 169, **kw) == paths.LAYER
    assert paths.bert_layer_fwd(SW, True, False, True, 60, 128, 169, **kw) == paths.OPS                   # rows of whole 16-byte vectors
    assert paths.stack_call(SW, True, 64, 128, 169, adapter_seq=True) == paths.STACK
    assert paths.stack_call(SW, True, 64, 128, 169) == paths.LAYER
    assert paths.stack_call(SW, False, 64, 128, 169, adapter_seq=True) == paths.LAYER


def test_what_still_sends_an_adapted_layer_to_the_op_by_op_path():
    kw = dict(adapters=True, adapter_seq=True)
    timed, no_seq, no_stack = SW._replace(timer=True), SW._replace(layer_seq=False), SW._replace(stack_seq=False)
    for sw in (timed, no_seq):
        assert paths.unimol_layer_fwd(sw, True, True, 512, 64, **kw) == paths.OPS
        assert paths.unimol_tower_bwd(sw, True, 2, 0, True, True, 512, 2048, 4096, [False, False], adapter_seq=True) == paths.OPS
        assert paths.bert_tower_fwd(sw, True, True, 6, 4096, **kw) == paths.LAYER
        for self_attn in (True, False):
            assert paths.bert_layer_fwd(sw, self_attn, False, True, 512, 2048, 4096, **kw) == paths.OPS
    assert paths.unimol_tower_fwd(no_stack, paths.LAYER, True, 15, 4096, False, True, **kw) == paths.LAYER
    assert paths.bert_tower_fwd(no_stack, True, True, 6, 4096, **kw) == paths.LAYER
    # a trainable base parameter (or MMDTI_LORA_SEQ=0): adapter_seq_ok says no, and every answer is the one without the keyword
    off = dict(adapters=True, adapter_seq=paths.adapter_seq_ok(True, [False, True], [True, True]))
    assert paths.unimol_layer_fwd(SW, True, True, 512, 64, **off) == paths.OPS
    assert paths.unimol_tower_fwd(SW, paths.LAYER, True, 15, 4096, False, True, **off) == paths.LAYER
    assert paths.unimol_layer_bwd(paths.LAYER, True, False, False, **off) == paths.OPS
    assert paths.bert_tower_fwd(SW, True, True, 6, 4096, **off) == paths.LAYER
    assert paths.bert_layer_fwd(SW, True, False, True, 512, 2048, 4096, **off) == paths.OPS


def test_the_defaults_are_the_answers_of_before():
    assert paths.unimol_layer_fwd(SW, True, True, 512, 64, adapters=True) == paths.OPS
    assert paths.unimol_tower_fwd(SW, paths.LAYER, True, 15, 4096, False, True, adapters=True) == paths.LAYER
    assert paths.unimol_layer_bwd(paths.LAYER, True, False, True, adapters=True) == paths.OPS
    assert paths.bert_tower_fwd(SW, True, True, 6, 4096, adapters=True) == paths.LAYER
    assert paths.bert_layer_fwd(SW, True, True, True, 512, 2048, 4096, adapters=True) == paths.OPS
    # adapter_seq without adapters changes nothing either
    assert paths.unimol_layer_fwd(SW, True, True, 512, 64, adapter_seq=True) == paths.LAYER
    assert paths.unimol_layer_bwd(paths.LAYER, True, True, True, adapter_seq=True) == paths.OPS           # (held weight gradients)
    assert paths.bert_layer_fwd(SW, True, False, True, 512, 2048, 4096, adapter_seq=True) == paths.OPS
    assert len(paths.Switches._fields) == 7


def test_the_switch_is_on_unless_the_environment_says_0():
    from mmdti_hip import functional as Fn
    assert Fn.LORA_SEQ is (os.environ.get("MMDTI_LORA_SEQ", "1") != "0")
