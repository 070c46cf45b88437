"""The sequencers' named blocks (include/mmdti_hip.h: mmdti_*_run_t / _layer_t / _saved_t), host side: the ctypes classes _abi builds
from the header lay the fields out as a C compiler does, every field is reachable by name, every sequencer refuses a block that lacks a
pointer it needs BEFORE its first launch, the workspace sizes come from one arithmetic, and a library of another ABI version is refused."""
import ctypes
import os
import shutil
import subprocess
import sys

import pytest

from mmdti_hip import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x10000            # fake, 16-byte aligned device address: nothing here dereferences it
STRUCTS = ("mmdti_unimol_run_t", "mmdti_unimol_layer_t", "mmdti_unimol_saved_t", "mmdti_bert_run_t", "mmdti_bert_layer_t", "mmdti_bert_saved_t")


def _cc():
    cc = os.environ.get("HIPCC") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc"))
    assert cc, "no hipcc (the compiler the library itself is built with)"
    return cc


def test_header_declares_the_blocks():
    assert set(_abi.parse_structs()) == set(STRUCTS)


def test_ctypes_layout_is_the_c_compilers(tmp_path):
    structs = _abi.parse_structs()
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "mmdti_hip.h"', "int main(void) {"]
    for name, cls in structs.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f, _ in cls._fields_]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", str(tmp_path / "layout")
    src.write_text("\n".join(lines) + "\n")
    # compiled AS C: the header stays plain C
    subprocess.run([_cc(), "-x", "c", "-std=c11", "-Wall", "-Werror", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-600:]
    got = dict(l.split() for l in r.stdout.splitlines())
    want = {}
    for name, cls in structs.items():
        want[name] = str(ctypes.sizeof(cls))
        want.update({f"{name}.{f}": str(getattr(cls, f).offset) for f, _ in cls._fields_})
    assert got == want
    assert len(want) > 130           # (six structs of 13 to 34 fields: the program did print them)


def test_every_field_is_reachable_by_name():
    lib = _abi.lib()
    src = open(_abi.HEADER).read()
    for name in STRUCTS:
        cls = lib.struct(name)
        fields = [f for f, _ in cls._fields_]
        assert len(set(fields)) == len(fields) >= 13
        body = src[src.rindex("typedef struct", 0, src.index("} " + name)):src.index("} " + name)]
        for f in fields:
            assert f in body
        vals = {f: (1.5 if t is ctypes.c_float else 3) for f, t in cls._fields_}
        blk = cls(**vals)
        assert all(getattr(blk, f) == vals[f] for f in fields)
        with pytest.raises(AttributeError):
            cls(**{fields[0] + "_": 1})
        assert all(not getattr(cls(), f) for f in fields)          # a field left out is null / zero


# ---- what each sequencer needs of the blocks it takes (csrc/layers.hip) ------------------------------------------------------------------
UNI_RUN = dict(seed=1, M=128, B=2, N=64, H=32, D=256, F=256, ld=64, pair_layout=3, act_fwd=4, act_dx=5, ln_max_k=0, fwd_f16=0, scale=0.35, p_res=0.0,
               p_att=0.0)
BERT_RUN = dict(seed=1, Mq=128, Mk=128, B=2, Lq=64, Lk=64, heads=4, D=256, F=256, q_rows=0, act_fwd=4, act_dx=5, ln_max_k=0, fwd_f16=0, scale=0.125,
                p_hid=0.0, p_att=0.0, eps=1e-12)
UNI_FWD_P = "w_in w_out w_fc1 w_fc2 g_ln2 bt_ln2".split()
UNI_BWD_P = "wb_fc2 wb_fc1 wb_out wb_in g_ln2 g_ln1 dw_fc2 dw_fc1 dw_out dw_in".split()
UNI_FWD_S = "x h1 qkv s o x1 h2 m2 r2 u a".split()
BERT_FWD_P = "w_qkv w_o g_ln1 bt_ln1 w_i w_o2 g_ln2 bt_ln2".split()
BERT_BWD_P = "wb_qkv wb_o wb_i wb_o2 g_ln1 g_ln2 dw_qkv dw_o dw_i dw_o2".split()
BERT_FWD_S = "s1_32 s1_16 qkv ctx stats y a32 a16 am ar u i z zm zr".split()
# entry point -> (tower, required fields of the layer block, required fields of the saved block | None: the stack calls build it)
NEEDS = {
    "mmdti_unimol_layer_fwd": ("unimol", UNI_FWD_P, UNI_FWD_S),
    "mmdti_unimol_layer_bwd": ("unimol", UNI_BWD_P, UNI_FWD_S + ["m1", "r1"]),
    "mmdti_unimol_stack_fwd": ("unimol", UNI_FWD_P + ["g_ln1", "bt_ln1"], None),
    "mmdti_unimol_stack_bwd": ("unimol", UNI_BWD_P, None),
    "mmdti_bert_layer_fwd": ("bert", BERT_FWD_P, BERT_FWD_S),
    "mmdti_bert_cross_layer_fwd": ("bert", BERT_FWD_P + ["w_q"], BERT_FWD_S + ["s2_16", "q"]),
    "mmdti_bert_layer_bwd": ("bert", BERT_BWD_P, "s1_16 qkv ctx stats y a16 am ar u i z zm zr".split()),
    "mmdti_bert_cross_layer_bwd": ("bert", "wb_qkv wb_q wb_o wb_i wb_o2 g_ln1 g_ln2".split(), "q qkv stats y am ar u z zm zr".split()),
    "mmdti_bert_stack_fwd": ("bert", BERT_FWD_P, None),
    "mmdti_bert_stack_bwd": ("bert", BERT_BWD_P, None),
}
NL = 2


def _pointers(cls, without=None):
    """A block whose every pointer field holds a dummy address -- except `without`."""
    return cls(**{f: PTR for f, t in cls._fields_ if t is ctypes.c_void_p and f != without}, **({"lddw_qkv": 256} if hasattr(cls, "lddw_qkv") else {}))


def _call(lib, name, run, layers, saved):
    """Call `name` with the three blocks; every other pointer a dummy, sizes generous, no side stream."""
    args = []
    for argname, t in zip(lib.protos[name][2], lib.protos[name][1]):
        if argname == "run":
            args.append(ctypes.addressof(run))
        elif argname in ("layer", "layers"):
            args.append(ctypes.addressof(layers))
        elif argname == "saved":
            args.append(ctypes.addressof(saved))
        elif argname in ("dw_stream", "events"):
            args.append(0)
        elif t is ctypes.c_void_p:
            args.append(PTR)
        elif t is ctypes.c_longlong:
            args.append(1 << 40)                 # arena / workspace / slab bytes
        elif t is ctypes.c_float:
            args.append(1e-5)
        else:
            args.append({"nl": NL, "next_mode": 1}.get(argname, 1))
    getattr(lib, name)(*args)


def test_struct_taking_entry_points_are_the_twelve_minus_the_queries():
    lib = _abi.lib()
    taking = {n for n, (_, _, argnames) in lib.protos.items() if "run" in argnames}
    assert taking == set(NEEDS)


@pytest.mark.parametrize("name", sorted(NEEDS))
def test_a_missing_pointer_is_refused_before_any_launch(name):
    """Complete blocks but for ONE required pointer: refused by the argument check (a complete block is never passed: it would launch)."""
    lib = _abi.lib()
    tower, need_p, need_s = NEEDS[name]
    run = lib.struct(f"mmdti_{tower}_run_t")(**(UNI_RUN if tower == "unimol" else BERT_RUN))
    P, S = lib.struct(f"mmdti_{tower}_layer_t"), lib.struct(f"mmdti_{tower}_saved_t")
    stack = need_s is None
    cases = [("layer", f) for f in need_p] + [("saved", f) for f in need_s or ()]
    assert len(cases) >= 6
    for which, field in cases:
        assert getattr(P if which == "layer" else S, field).size == 8           # (a pointer field)
        # (a stack call: the gap sits in the LAST layer's block -- the layers under it must not have been launched by then)
        layers = (P * NL)(*[_pointers(P, field if which == "layer" and l == NL - 1 else None) for l in range(NL)]) if stack else _pointers(
            P, field if which == "layer" else None)
        saved = _pointers(S, field if which == "saved" else None)
        with pytest.raises(_abi.MMDTIError, match=r"null (argument|parameter)"):
            _call(lib, name, run, layers, saved)
    # ... and a null block itself
    if not stack:
        with pytest.raises(_abi.MMDTIError, match="null block"):
            getattr(lib, name)(0, ctypes.addressof(run), 0, *([0] * (len(lib.protos[name][1]) - 3)))


# ---- one arithmetic for the workspace sizes ------------------------------------------------------------------------------------------------
def _slab(lib, D, F, rows):
    tiles = (D // 256) * (F // 256) * 2 + (D // 256) ** 2 * 4
    return lib._dll.mmdti_linear_dw_grouped_splits(tiles, rows) * (2 * D * F + 4 * D * D) * 4


# the three formulas functional.py carried before the library answered the question (M rows; nrow: rows of the attention statistics)
def _unimol_layer_ws_bytes(M, D, F, slab):
    return (M * F + 7 * M * D) * 2 + M * D * 4 + slab


def _bert_layer_ws_bytes(Mq, D, F, nrow, slab):
    return (Mq * F + 7 * Mq * D) * 2 + Mq * D * 4 + (nrow * 4 + 15) // 16 * 16 + slab


def _bert_cross_layer_ws_bytes(Mq, D, nrow):
    return 4 * Mq * D + 4 * Mq * D + (nrow * 4 + 15) // 16 * 16


# (M, D, F, s_bytes) -> (slab bytes, arena bytes per layer, stack workspace bytes): recorded from the library before the structs
UNIMOL_LAYOUTS = {
    (33280, 512, 2048, 1 << 20): (62914560, 614998016, 1250426880),
    (128, 256, 256, 4096): (1572864, 792576, 4915200),
    (4097, 512, 1024, 12345): (67108864, 58813696, 255882240),
}
# (Mq, D, F, nrow) -> the same; stats_bytes = 8 nrow.  nrow: B * heads * L dense (130 x 8 x 256; 2 x 4 x 64), heads * q_rows packed (12 x 1000)
BERT_LAYOUTS = {
    (33280, 512, 2048, 266240): (62914560, 752394240, 643317760),
    (128, 256, 256, 512): (1572864, 1054720, 2492416),
    (1000, 768, 3072, 12000): (56623104, 33904384, 82783232),
}


def test_layer_workspace_bytes_come_from_the_librarys_one_arithmetic():
    lib = _abi.lib()
    out = (ctypes.c_longlong * 4)()
    for (M, D, F, s_bytes), (slab, stride, ws) in UNIMOL_LAYOUTS.items():
        assert _slab(lib, D, F, M) == slab
        lib.mmdti_unimol_stack_layout(M, D, F, s_bytes, slab, ctypes.addressof(out))
        assert (out[0], out[1]) == (stride, ws)
        assert out[2] == _unimol_layer_ws_bytes(M, D, F, slab)
    for (M, D, F, nrow), (slab, stride, ws) in BERT_LAYOUTS.items():
        assert _slab(lib, D, F, M) == slab
        lib.mmdti_bert_stack_layout(M, D, F, 8 * nrow, nrow, slab, ctypes.addressof(out))
        assert (out[0], out[1]) == (stride, ws)
        assert out[2] == _bert_layer_ws_bytes(M, D, F, nrow, slab)
        assert out[3] == _bert_cross_layer_ws_bytes(M, D, nrow)


def test_the_host_asks_the_library_once_per_shape():
    from mmdti_hip import functional as Fn
    for gone in ("_unimol_layer_ws_bytes", "_bert_layer_ws_bytes", "_bert_cross_layer_ws_bytes"):
        assert not hasattr(Fn, gone)
    lib = _abi.lib()
    r = Fn._stack_layout("mmdti_bert_stack_layout", 1000, 768, 3072, 96000, 12000)
    slab = _slab(lib, 768, 3072, 1000)
    assert r == BERT_LAYOUTS[(1000, 768, 3072, 12000)][1:] + (slab, _bert_layer_ws_bytes(1000, 768, 3072, 12000, slab), _bert_cross_layer_ws_bytes(1000, 768, 12000))
    assert Fn._stack_layout("mmdti_bert_stack_layout", 1000, 768, 3072, 96000, 12000) is r          # cached
    r = Fn._stack_layout("mmdti_unimol_stack_layout", 128, 256, 256, 0)
    assert r[3] == _unimol_layer_ws_bytes(128, 256, 256, _slab(lib, 256, 256, 128))


# ---- the ABI version -----------------------------------------------------------------------------------------------------------------------
def test_header_and_library_agree_on_the_abi_version():
    lib = _abi.lib()
    assert lib.const["MMDTI_ABI_VERSION"] == 2 == lib._dll.mmdti_abi_version()


def test_a_library_of_another_abi_version_is_refused(tmp_path):
    src, so = tmp_path / "stub.c", str(tmp_path / "libstub.so")
    src.write_text("int mmdti_abi_version(void) { return %d; }\n" % (_abi.header_constants()["MMDTI_ABI_VERSION"] - 1))
    subprocess.run([_cc(), "-x", "c", "-shared", "-fPIC", str(src), "-o", so], check=True, timeout=300)
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from mmdti_hip import _abi\n"
            "try:\n"
            "    _abi.lib()\n"
            "except _abi.MMDTIError as e:\n"
            "    print('refused:', e)\n") % (ROOT, os.path.join(ROOT, "mm-dti_amd"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MMDTI_HIP_LIB=so), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("refused:") and "ABI version 1" in r.stdout and "declares 2" in r.stdout, (r.stdout[-400:], r.stderr[-400:])
