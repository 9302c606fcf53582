"""ctypes binding of libpd_hip.so — the C-ABI declared in include/*.h.

The HIP library is the product: there is NO fallback.  If the shared object is
missing or a symbol is absent this module raises, and every op built on it
raises with it (a GPU box must never silently run something else).
"""
import ctypes
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PD_LIB_PATH") or os.path.join(_HERE, "libpd_hip.so")   # PD_LIB_PATH: development A/B of two builds (tools/ab_bench.sh)
CSRC = os.path.join(_HERE, "csrc")

INCLUDE = os.path.join(os.path.dirname(_HERE), "include")           # the headers csrc/Makefile compiles against (-I../../include)

PD_F32, PD_F64, PD_BF16 = 0, 1, 2                                    # an enum of pd_msda.h: the reader binds #defines, not enumerators

_lib = None
_PROXY = None            # cmdbuf.Recording: while a region is being recorded load() hands out its recording proxy


class PdHipError(RuntimeError):
    pass


# ---- the binding is DERIVED from include/*.h: prototypes -> SIGNATURES, typedef'd structs -> struct(), integer #define PD_* -> const().
# The headers keep to a narrow C subset; whatever falls outside it raises here, nothing is skipped or guessed.
_SCALAR = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "int16_t": ctypes.c_int16, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
           "uint8_t": ctypes.c_uint8, "float": ctypes.c_float, "double": ctypes.c_double}
_NAME = re.compile(r"[A-Za-z_]\w*")


def _ctype(decl, where):
    """`type [name]` of a return value or parameter -> ctypes: `const char *` is c_char_p, every other pointer c_void_p"""
    if "*" in decl:
        return ctypes.c_char_p if [w for w in decl.split("*")[0].split() if w != "const"] == ["char"] else ctypes.c_void_p
    words = [w for w in decl.split() if w != "const"]
    if len(words) in (1, 2) and words[0] in _SCALAR and _NAME.fullmatch(words[-1]):
        return _SCALAR[words[0]]
    raise PdHipError(f"{where}: cannot classify the type in `{decl}`")


def _const_value(text, consts, where):
    """integer expression of decimal literals, known PD_* names, parentheses, unary minus and <<"""
    toks, pos = re.findall(r"\w+|<<|\S", text), 0

    def take():
        nonlocal pos
        pos += 1
        return toks[pos - 1] if pos <= len(toks) else ""

    def unary():
        t = take()
        if t == "-":
            return -unary()
        if t == "(":
            v = shift()
            if take() != ")":
                raise PdHipError(f"{where}: unbalanced parentheses in `{text}`")
            return v
        if t.isdigit() and (t == "0" or t[0] != "0"):
            return int(t)
        if t in consts:
            return consts[t]
        raise PdHipError(f"{where}: `{text}` is not an integer constant expression the binding can read (at `{t}`)")

    def shift():
        v = unary()
        while toks[pos:pos + 1] == ["<<"]:
            take()
            v <<= unary()
        return v
    v = shift()
    if pos != len(toks):
        raise PdHipError(f"{where}: `{text}` is not an integer constant expression the binding can read (at `{toks[pos]}`)")
    return v


def _fields(body, consts, where):
    """`const float *dY, *X; int32_t K, h, w; uint64_t a[PD_CMD_MAX_ARGS];` -> _fields_ (a pointer of any type is c_void_p)"""
    out = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.fullmatch(r"(?:const )?(\w+) (.+)", decl)
        if m is None:
            raise PdHipError(f"{where}: cannot classify the struct field `{decl}`")
        for d in m[2].split(","):
            d = d.replace(" ", "")
            arr = re.fullmatch(r"(\w+)\[(.+)\]", d)
            if d.startswith("*") and _NAME.fullmatch(d.lstrip("*")):
                out.append((d.lstrip("*"), ctypes.c_void_p))
            elif m[1] in _SCALAR and arr and _NAME.fullmatch(arr[1]):
                out.append((arr[1], _SCALAR[m[1]] * _const_value(arr[2], consts, where)))
            elif m[1] in _SCALAR and _NAME.fullmatch(d):
                out.append((d, _SCALAR[m[1]]))
            else:
                raise PdHipError(f"{where}: cannot classify the struct field `{decl}`")
    return out


def read_headers(include_dir):
    """-> (signatures {name: (restype, [argtypes])}, structs {name: ctypes.Structure subclass}, consts {PD_NAME: int}) of *.h there"""
    sigs, structs, consts = {}, {}, {}
    for fname in sorted(f for f in os.listdir(include_dir) if f.endswith(".h")):
        with open(os.path.join(include_dir, fname)) as fh:
            text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", fh.read(), flags=re.S)           # comments quote calls: they go first
        text = re.sub(r"#\s*ifdef __cplusplus\b.*?#\s*endif", " ", text, flags=re.S)   # the extern "C" braces
        code = []
        for line in text.split("\n"):
            if not line.lstrip().startswith("#"):
                code.append(line)
                continue
            m = re.fullmatch(r"\s*#\s*(include|ifndef|endif|define)\b\s*(\w*)(.*)", line)
            if m is None or line.rstrip().endswith("\\") or (m[1] == "define" and m[3].startswith("(")):
                raise PdHipError(f"{fname}: preprocessor line the binding cannot read: `{line.strip()}`")
            if m[1] == "define" and m[2].startswith("PD_") and m[3].strip():           # no value: an include guard
                consts[m[2]] = _const_value(m[3], consts, fname)
        text, depth, start = "\n".join(code), 0, 0
        for i, ch in enumerate(text):
            depth += (ch == "{") - (ch == "}")
            if ch != ";" or depth:
                continue
            s, start = " ".join(text[start:i].split()), i + 1
            st = re.fullmatch(r"typedef struct ?\w* ?\{(.*)\} ?(\w+)", s)
            fn = re.fullmatch(r"([\w ]+?[ *]+)(pd_\w+) ?\((.*)\)", s)
            if st:
                structs[st[2]] = type(st[2], (ctypes.Structure,), {"_fields_": _fields(st[1], consts, f"{fname}: {st[2]}")})
            elif fn:
                args = [] if fn[3].strip() == "void" else [_ctype(a, f"{fname}: {fn[2]}") for a in fn[3].split(",")]
                sigs[fn[2]] = (None if fn[1].strip() == "void" else _ctype(fn[1], f"{fname}: {fn[2]}"), args)
            elif s and not s.startswith("enum "):
                raise PdHipError(f"{fname}: declaration the binding cannot read: `{s}`")
        if text[start:].strip():
            raise PdHipError(f"{fname}: declaration without its `;`: `{' '.join(text[start:].split())}`")
    return sigs, structs, consts


SIGNATURES, _STRUCTS, _CONSTS = read_headers(INCLUDE)                # name -> (restype, argtypes) of every exported function


def struct(name):
    """the ctypes.Structure of a struct typedef'd in include/*.h (one class per name, made at import)"""
    return _STRUCTS[name]


def const(name):
    """the value of an integer `#define PD_*` of include/*.h"""
    return _CONSTS[name]


ABI_VERSION = const("PD_ABI_VERSION")


def build(force=False, verbose=False):
    """Compile every csrc/*.hip for gfx950 into libpd_hip.so (in-tree)."""
    args = ["make", "-C", CSRC, "-j4"] + (["-B"] if force else [])
    out = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or out.returncode != 0:
        print(out.stdout)
    if out.returncode != 0:
        raise PdHipError("building libpd_hip.so failed")
    return LIB_PATH


def real():
    """the library itself, never the recording proxy"""
    return _lib if _lib is not None else load()


def load():
    global _lib
    if _PROXY is not None:
        return _PROXY
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PdHipError(
            f"{LIB_PATH} is missing: the HIP extension has not been built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C partdistillation_amd/csrc`). "
            "partdistillation_amd has no CPU or PyTorch fallback.")
    # PyTorch ships its own libamdhip64 / libhsa-runtime64; libpd_hip.so is linked against the same SONAME.  Import torch
    # FIRST so that the process has ONE HIP runtime - the one torch's streams and allocations live in.  (Loaded the other way
    # round, the system runtime wins and every launch fails with "no ROCm-capable device is detected".)
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise PdHipError(f"libpd_hip.so does not export `{name}` (stale build?)") from e
        fn.restype, fn.argtypes = res, args
    if lib.pd_abi_version() != ABI_VERSION:
        raise PdHipError(f"libpd_hip.so ABI {lib.pd_abi_version()} != binding {ABI_VERSION}: rebuild")
    # development knobs of the kernels (tools/ab_bench.sh): PD_DEBUG_SET="key=value,key=value" -> pd_debug_set at load
    for kv in filter(None, os.environ.get("PD_DEBUG_SET", "").split(",")):
        k, v = kv.split("=")
        if lib.pd_debug_set(k.encode(), int(v)) != 0:
            raise PdHipError(f"PD_DEBUG_SET: unknown key `{k}`")
    _lib = lib
    return lib


def current_stream():
    """raw hipStream_t of torch's current stream on the current device.  torch.cuda.current_stream().cuda_stream costs
    ~9 us of host time per call (Stream object construction); the two C calls below ~0.5 us - it is called once per launch."""
    import torch
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


def check(rc):
    if rc != 0:
        raise PdHipError(load().pd_last_error().decode() or f"libpd_hip error {rc}")
