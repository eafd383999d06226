"""ctypes binding of libpzn.so — the C ABI declared in include/pzn.h.

The library is built ahead of time by ``python -m puzzlenet_amd.build`` (hipcc,
gfx950) and lives next to this file.  There is NO fallback: if the shared
object is missing, or a call returns a non-zero status, this raises.

The binding table and the ABI's integer constants are read from include/pzn.h
when this module is imported (parse_header): the header is their only statement.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpzn.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "pzn.h")

_c_f = ctypes.c_void_p      # device pointers travel as raw addresses
_c_i = ctypes.c_int
_c_sz = ctypes.c_size_t
_c_fl = ctypes.c_float
_c_ll = ctypes.c_longlong
_SCALARS = {"int": _c_i, "float": _c_fl, "double": ctypes.c_double, "long long": _c_ll, "size_t": _c_sz}


class PznError(RuntimeError):
    pass


class PznUnsupported(PznError):
    """status PZN_EUNSUPPORTED: the entry point does not take this shape / alignment; composed entry points
    document the alternative path."""


_INT = r"[-+]?(?:0[xX][0-9a-fA-F]+|\d+)"


def parse_header(text, path="<header>"):
    """The C ABI a header declares -> (functions, constants): functions[name] = (restype, [argtypes], [parameters as
    written, e.g. "const float* xyz"]), constants[NAME] = int for every enumerator and `#define NAME <integer>`.
    The grammar is what include/pzn.h uses and no more: `typedef void* T;`, `enum { NAME = <integer>, ... };`,
    `#define NAME <integer>` and prototypes over int / float / double / long long / size_t and pointers, inside
    `extern "C" { }`.  Anything else is an error, never a guess: a scalar bound as the wrong type is a wild pointer
    on the device."""
    def fail(decl, why):
        raise PznError(f"{path}: cannot bind `{' '.join(decl.split())}`: {why}")

    functions, constants, pointer_types = {}, {}, set()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    code = []
    for line in text.splitlines():
        if line.lstrip().startswith("#"):
            m = re.fullmatch(rf"\s*#\s*define\s+(\w+)\s+({_INT})\s*", line)
            if m:
                constants[m.group(1)] = int(m.group(2), 0)
        else:
            code.append(line)
    text, wrapped = re.subn(r'extern\s+"C"\s*\{', " ", "\n".join(code))
    *statements, rest = text.split(";")
    if rest.strip() != "}" * wrapped:
        fail(rest, "declaration without a closing `;`")

    def ctype(decl, kind, result=False):
        kind = " ".join(kind.replace("*", " * ").split())
        if result and kind == "const char *":
            return ctypes.c_char_p
        if not result and ("*" in kind or kind in pointer_types):
            return ctypes.c_void_p
        scalar = kind[6:] if kind.startswith("const ") else kind
        if scalar not in _SCALARS:
            fail(decl, f"no binding for the type `{kind}`")
        return _SCALARS[scalar]

    for decl in statements:
        decl = decl.strip()
        m = re.fullmatch(r"typedef\s+void\s*\*\s*(\w+)", decl)
        if m:
            pointer_types.add(m.group(1))
            continue
        m = re.fullmatch(r"enum\s*\{(.*)\}", decl, flags=re.S)
        if m:
            for item in m.group(1).split(","):
                e = re.fullmatch(rf"\s*(\w+)\s*=\s*({_INT})\s*", item)
                if not e:
                    fail(decl, f"enumerator `{item.strip()}` is not NAME = <integer>")
                constants[e.group(1)] = int(e.group(2), 0)
            continue
        m = re.fullmatch(r"([\w\s*]+?)\b(pzn_\w+)\s*\(([^()]*)\)", decl)
        if not m:
            fail(decl, "not a typedef, an enum or a prototype `<result> pzn_name(<parameters>)`")
        result, name, params = m.groups()
        if name in functions:
            fail(decl, "declared twice")
        params = [] if params.strip() == "void" else [" ".join(p.split()) for p in params.split(",")]
        argtypes = []
        for p in params:
            pm = re.fullmatch(r"(.*[\s*])\w+", p)
            if not pm:
                fail(decl, f"parameter `{p}` is not `<type> <name>`")
            argtypes.append(ctype(decl, pm.group(1)))
        functions[name] = (ctype(decl, result, result=True), argtypes, params)
    return functions, constants


def read_header(path=HEADER_PATH):
    try:
        with open(path) as f:
            text = f.read()
    except OSError as e:
        raise PznError(f"{path}: the header that declares the C ABI cannot be read ({e})") from None
    return parse_header(text, path)


_functions, CONSTANTS = read_header()
SIGNATURES = {name: (res, args) for name, (res, args, _) in _functions.items()}    # name -> (restype, argtypes)
PARAMS = {name: params for name, (_, _, params) in _functions.items()}              # name -> parameters as written

_lib = None


def load():
    """Load libpzn.so (raises if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PznError(
                f"{LIB_PATH} is missing: build it with `python -m puzzlenet_amd.build` "
                "(hipcc --offload-arch=gfx950). There is no CPU or eager fallback.")
        # torch ships its own libamdhip64.so.7; device pointers and streams handed to the
        # C ABI belong to THAT runtime instance, so it must be the one libpzn.so binds to.
        # Same SONAME => whichever copy is loaded first wins; load torch's first.
        import torch  # noqa: F401
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)          # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def check(status, what):
    if status != 0:
        msg = load().pzn_strerror(status).decode()
        unsupported = status == CONSTANTS["PZN_EUNSUPPORTED"]
        raise (PznUnsupported if unsupported else PznError)(f"{what} failed: {msg} (status {status})")


_FN = {}


def call(name, *args):
    """Invoke an int-status entry point and raise on error."""
    fn = _FN.get(name)
    if fn is None:
        fn = _FN[name] = getattr(load(), name)
    status = fn(*args)
    if status != 0:
        check(status, name)
