"""ctypes binding of libmmdti_hip.so -- the only way the host package reaches the kernels.

The prototypes are parsed from ``include/mmdti_hip.h`` (the single source of truth for the C ABI), so the Python
side cannot drift from the header.  There is NO fallback: if the shared library is missing or a symbol the header
declares is absent, importing this module raises.
"""
import ctypes
import os
import re

# torch must load ITS bundled HIP runtime (torch/lib/libamdhip64.so) before libmmdti_hip.so is dlopen'ed: both have the
# same SONAME, and the first one loaded serves the whole process.  Loading the system copy first leaves torch and the
# kernels on different runtimes ("no ROCm-capable device is detected").
import torch  # noqa: F401  (plumbing: device memory + streams)

_HERE = os.path.dirname(os.path.abspath(__file__))
REPO_ROOT = os.path.dirname(os.path.dirname(_HERE))
HEADER = os.path.join(REPO_ROOT, "include", "mmdti_hip.h")
LIB_PATH = os.environ.get("MMDTI_HIP_LIB", os.path.join(_HERE, "lib", "libmmdti_hip.so"))


class MMDTIError(RuntimeError):
    pass


def _ctype(decl: str):
    d = decl.strip()
    if "*" in d or d.startswith("mmdti_stream_t"):
        return ctypes.c_void_p
    d = re.sub(r"\b[A-Za-z_][A-Za-z_0-9]*$", "", d).strip() if len(d.split()) > 1 else d   # drop the parameter name
    d = d.replace("const", "").strip()
    table = {
        "int": ctypes.c_int, "unsigned int": ctypes.c_uint, "long long": ctypes.c_longlong,
        "unsigned long long": ctypes.c_ulonglong, "float": ctypes.c_float, "void": None,
    }
    if d not in table:
        raise MMDTIError(f"mmdti_hip.h: unsupported parameter type in {decl!r}")
    return table[d]


def _source(path):
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return re.sub(r"//[^\n]*", "", src)


def parse_structs(path: str = HEADER, tagged: bool = False):
    """-> {name: ctypes.Structure subclass} for every `typedef struct { ... } mmdti_*_t;` of the header, fields in header order.  A
    declaration is `type a, b;` or -- pointers -- `type *a, *b;` / `type* a;`; no arrays, bitfields or nested structs.
    tagged: also the blocks declared with a struct tag, `typedef struct mmdti_x { ... } mmdti_x_t;` (the adapted sequencers').  The
    default leaves them out for one reason only: callers that enumerate the six blocks of the plain sequencers -- the layout and
    null-pointer checks of tests/test_layer_structs_cpu.py pin that set -- keep their answer.  lib().struct(name) knows all of them;
    tests/test_lora_seq_cpu.py holds the tagged ones to the C compiler's layout."""
    structs = {}
    for tag, body, name in re.findall(r"typedef\s+struct\s*(mmdti_[a-z0-9_]+)?\s*\{([^{}]*)\}\s*(mmdti_[a-z0-9_]+_t)\s*;", _source(path)):
        if tag and not tagged:
            continue
        fields = []
        for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
            first, *more = [d.strip() for d in decl.split(",")]
            base = re.sub(r"[A-Za-z_][A-Za-z_0-9]*$", "", first).replace("*", " ")
            for d in [first] + more:
                if not re.fullmatch(r"[A-Za-z_0-9 ]*\*?\s*[A-Za-z_][A-Za-z_0-9]*", d):
                    raise MMDTIError(f"mmdti_hip.h: unsupported field {d!r} in {name}")
                field = re.findall(r"[A-Za-z_][A-Za-z_0-9]*", d)[-1]
                fields.append((field, _ctype(f"{base} {'*' if '*' in d else ''}{field}")))
        # (no instance dictionary: ctypes would otherwise take a misspelt keyword for a new Python attribute and leave the field null)
        structs[name] = type(name, (ctypes.Structure,), {"__slots__": (), "_fields_": fields})
    return structs


def parse_header(path: str = HEADER):
    """-> {name: (restype, [argtypes], [argnames])} for every function the header declares.  A struct-pointer parameter is a plain
    address (c_void_p): pass ctypes.addressof of a block built from lib().struct(name)."""
    src = _source(path)
    protos = {}
    for m in re.finditer(r"(const\s+char\s*\*|int)\s+(mmdti_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        ret, name, args = m.group(1), m.group(2), m.group(3)
        args = " ".join(args.split())
        if args in ("void", ""):
            argtypes, argnames = [], []
        else:
            parts = [a.strip() for a in args.split(",")]
            argtypes = [_ctype(a) for a in parts]
            argnames = [re.findall(r"[A-Za-z_][A-Za-z_0-9]*", a)[-1] for a in parts]
        protos[name] = (ctypes.c_char_p if "char" in ret else ctypes.c_int, argtypes, argnames)
    if not protos:
        raise MMDTIError(f"no prototypes found in {path}")
    return protos


def header_constants(path: str = HEADER):
    return {k: int(v) for k, v in re.findall(r"#define\s+(MMDTI_[A-Z0-9_]+)\s+(\d+)", open(path).read())}


class _Lib:
    def __init__(self):
        if not os.path.exists(LIB_PATH):
            raise MMDTIError(
                f"libmmdti_hip.so not found at {LIB_PATH}: build it with `python __graft_entry__.py` "
                f"(make -C mm-dti_amd/csrc).  There is no CPU fallback for the product path.")
        self._dll = ctypes.CDLL(LIB_PATH)
        self.protos = parse_header()
        self.structs = parse_structs(tagged=True)
        self.const = header_constants()
        try:
            version = self._dll.mmdti_abi_version()
        except AttributeError as e:
            raise MMDTIError(f"{LIB_PATH} does not export mmdti_abi_version") from e
        if version != self.const["MMDTI_ABI_VERSION"]:
            raise MMDTIError(f"{LIB_PATH} was built for ABI version {version}, include/mmdti_hip.h declares "
                             f"{self.const['MMDTI_ABI_VERSION']}: rebuild it (make -C mm-dti_amd/csrc)")
        for name, (restype, argtypes, _) in self.protos.items():
            try:
                fn = getattr(self._dll, name)
            except AttributeError as e:
                raise MMDTIError(f"{LIB_PATH} does not export {name} declared in include/mmdti_hip.h") from e
            fn.restype = restype
            fn.argtypes = argtypes
        self._last_error = self._dll.mmdti_last_error

    def struct(self, name):
        """The ctypes class of the header's `name`: build a block by keyword (an unknown field name is an AttributeError); a field left out is
        null, which every entry point that needs it refuses before its first launch."""
        return self.structs[name]

    def call(self, name, *args):
        rc = getattr(self._dll, name)(*args)
        if rc != 0:
            msg = self._last_error()
            raise MMDTIError(f"{name} failed (code {rc}): {msg.decode() if msg else '?'}")

    def __getattr__(self, name):
        # (reached once per symbol: the checked caller is cached on the instance, so later lookups skip this method)
        if name.startswith("mmdti_"):
            fn = getattr(self._dll, name)
            if self.protos[name][0] is ctypes.c_int and name != "mmdti_abi_version":
                last_error = self._last_error

                def checked(*a, _fn=fn, _name=name):
                    rc = _fn(*a)
                    if rc != 0:
                        msg = last_error()
                        raise MMDTIError(f"{_name} failed (code {rc}): {msg.decode() if msg else '?'}")
                fn = checked
            self.__dict__[name] = fn
            return fn
        raise AttributeError(name)


_lib = None


def lib() -> _Lib:
    global _lib
    if _lib is None:
        _lib = _Lib()
    return _lib
