"""ctypes loader for libp3hip.so — the only compute backend of this package.

There is deliberately NO fallback: if the HIP extension is missing or a symbol is absent the import
of any op fails loudly (RuntimeError), so a silent eager/PyTorch path can never masquerade as the product.

include/p3hip.h is the single declaration of the C-ABI: declare() gives every function of a loaded library the
argtypes / restype of its prototype there, so that ctypes converts and checks each argument (a bare Python int
reaches an int64_t parameter as 64 bits, a c_int there is refused) and no call site wraps scalars or sets a restype.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# P3HIP_LIB selects another build of the same library (A/B runs of two kernel variants on one box: tools/ab.sh)
LIB_PATH = os.environ.get("P3HIP_LIB") or os.path.join(_HERE, "libp3hip.so")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "p3hip.h")
_lib = None

_SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "unsigned int": ctypes.c_uint, "int64_t": ctypes.c_int64,
            "float": ctypes.c_float, "double": ctypes.c_double}


class P3Error(RuntimeError):
    pass


def _ctype(decl, name, ret=False):
    """ctypes class of one parameter ("const float* x", "int64_t n", "float taps[4]") or return type of prototype `name`"""
    if "*" in decl or "[" in decl or "hipStream_t" in decl:       # any pointer (struct pointers too): byref(), ctypes arrays, None and integers pass
        return ctypes.c_char_p if ret and "char" in decl else ctypes.c_void_p
    words = decl.replace("const", " ").split()
    key = " ".join(words if ret else words[:-1])                   # a parameter's last word is its name
    if ret and key == "void":
        return None
    if key not in _SCALARS:
        raise P3Error(f"{HEADER}: cannot map the type of '{decl.strip()}' in the prototype of {name} to ctypes")
    return _SCALARS[key]


def prototypes(header=None):
    """{name: (restype, [argtypes])} of every `ret p3_name(args);` in include/p3hip.h (not a C parser: the header keeps to one-statement prototypes)"""
    text = open(header or HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)              # comments
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)                # preprocessor lines
    text = re.sub(r"typedef\s+struct\s*\{.*?\}\s*\w+\s*;", " ", text, flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"([\w\s]+?[\s*]+)(p3_\w+)\s*\(([^;{}()]*)\)\s*;", text):
        params = [] if args.strip() in ("", "void") else args.split(",")
        out[name] = (_ctype(ret, name, ret=True), [_ctype(p, name) for p in params])
    return out


def declare(cdll):
    """set restype / argtypes of every function include/p3hip.h declares on `cdll`; a declared symbol the library lacks is an error"""
    for name, (restype, argtypes) in prototypes().items():
        try:
            fn = getattr(cdll, name)
        except AttributeError:
            raise P3Error(f"{cdll._name} does not export {name}, which {HEADER} declares: rebuild the library") from None
        fn.restype, fn.argtypes = restype, argtypes
    return cdll


def load(path):
    """ctypes.CDLL(path) declared from the header: for callers that open a build of the library themselves (tests, A/B tools)"""
    return declare(ctypes.CDLL(path))


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise P3Error(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950). There is no CPU / eager fallback.")
        _lib = load(LIB_PATH)
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().p3_last_error_string().decode()
        raise P3Error(f"{what} failed with code {rc}: {msg}")
