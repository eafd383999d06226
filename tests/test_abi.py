"""CPU: libpzn.so builds (hipcc cross-compile, no GPU needed), loads, and exports
exactly the entry points include/pzn.h declares.  No compute call is made here."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "pzn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(pzn_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib_path():
    from puzzlenet_amd import build
    return build.build()


def test_header_declares_entry_points():
    names = _declared()
    assert "pzn_fps_f32" in names and "pzn_knn_f32" in names and "pzn_emd_fused_f32" in names
    assert len(names) >= 15


def test_library_exports_every_declared_symbol(lib_path):
    lib = ctypes.CDLL(lib_path)
    missing = [n for n in _declared() if not hasattr(lib, n)]
    assert not missing, missing


def test_binding_table_matches_header(lib_path):
    from puzzlenet_amd import _lib
    assert sorted(_lib.SIGNATURES) == _declared()
    lib = _lib.load()
    assert lib.pzn_version() >= 100
    assert lib.pzn_strerror(-1).decode().startswith("invalid")
    assert lib.pzn_emd_workspace_bytes(2, 8, 8) > 0


def test_derived_table_binds_every_type_form_as_pinned():
    """The table is read from the header (_lib.parse_header); one entry per type form is written out here by hand."""
    from puzzlenet_amd import _lib
    i, fl, sz, ll, p = _lib._c_i, _lib._c_fl, _lib._c_sz, _lib._c_ll, ctypes.c_void_p
    assert _lib._c_f is p
    pinned = {
        "pzn_strerror": (ctypes.c_char_p, [i]),
        "pzn_emd_workspace_bytes": (sz, [i, i, i]),
        "pzn_ktimer_row": (i, [i, p, i, p, p]),                                    # char*, int*, double*
        "pzn_ball_query_f32": (i, [fl, i, p, p, i, i, i, p, p]),
        "pzn_point_mlp3_fwd_f32": (i, [p, ll, i, p, i, p, i, p, p, p, p, i, i, p, p, p, p]),
        "pzn_avg4_f32": (i, [p, p, p, p, sz, p, p]),
        "pzn_attn_fused_fwd": (i, [i] + [p] * 6 + [i] + [p] * 5 + [i, fl, p]),      # `const float* const*`, float, stream
        "pzn_sa_level_bwd_pt_f32": (i, [p] * 12 + [i] * 6 + [p] * 5 + [i, p, p]),
    }
    for name, (res, args) in pinned.items():
        got_res, got_args = _lib.SIGNATURES[name]
        assert got_res is res, (name, got_res)
        assert len(got_args) == len(args) and all(a is b for a, b in zip(got_args, args)), (name, got_args)
        assert len(_lib.PARAMS[name]) == len(args)
    assert len(_lib.SIGNATURES["pzn_sa_level_bwd_pt_f32"][1]) == 26
    assert _lib.PARAMS["pzn_ktimer_row"] == ["int i", "char* name", "int cap", "int* launches", "double* ms"]
    assert len(_lib.SIGNATURES) == len(_declared())
    assert _lib.CONSTANTS == {"PZN_OK": 0, "PZN_EINVAL": -1, "PZN_ELAUNCH": -2, "PZN_EUNSUPPORTED": -3, "PZN_ENODEVICE": -4,
                              "PZN_BOUNDARY_CE_LOSS_FLOATS": 513}


_SMALL_HEADER = """
/* a comment with f(int x); and (parentheses); inside */
#ifndef SMALL_H_
#define SMALL_H_
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef void* pzn_stream_t; /* opaque; 0 = null stream */
enum {
  PZN_OK = 0,      /* fine, (really); */
  PZN_EBAD = -7,
  PZN_MASK = 0x10
};
#define PZN_FLOATS 513
#define PZN_NEG -2
int pzn_none(void);   // a line comment with pzn_ghost(int a);
const char* pzn_text(int status);
size_t
pzn_spread(const float* const* x,   /* one per problem (n of them); */
           long long M, const double* d,
           float scale, double eps, size_t n, const int v, pzn_stream_t stream);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_on_a_small_header():
    from puzzlenet_amd import _lib
    p = ctypes.c_void_p
    fns, consts = _lib.parse_header(_SMALL_HEADER)
    assert sorted(fns) == ["pzn_none", "pzn_spread", "pzn_text"]                   # nothing out of a comment
    assert fns["pzn_none"] == (_lib._c_i, [], [])                                  # (void)
    assert fns["pzn_text"] == (ctypes.c_char_p, [_lib._c_i], ["int status"])
    res, args, params = fns["pzn_spread"]                                          # four lines
    assert res is _lib._c_sz
    assert args == [p, _lib._c_ll, p, _lib._c_fl, ctypes.c_double, _lib._c_sz, _lib._c_i, p]
    assert params == ["const float* const* x", "long long M", "const double* d", "float scale", "double eps", "size_t n",
                      "const int v", "pzn_stream_t stream"]
    assert consts == {"PZN_OK": 0, "PZN_EBAD": -7, "PZN_MASK": 16, "PZN_FLOATS": 513, "PZN_NEG": -2}   # no include guard


@pytest.mark.parametrize("text,names", [
    ("int pzn_a(unsigned int n);", ["pzn_a", "unsigned int"]),                     # a scalar outside the set: never `int`
    ("int pzn_a(int64_t n);", ["pzn_a", "int64_t"]),
    ("int pzn_a(pzn_stream_t stream);", ["pzn_a", "pzn_stream_t"]),                # its typedef is not in this header
    ("short pzn_a(int n);", ["pzn_a", "short"]),
    ("float* pzn_a(int n);", ["pzn_a", "float *"]),                                # a pointer result other than const char*
    ("int pzn_a(int);", ["pzn_a", "`int`"]),                                       # a parameter without a name
    ("int pzn_a(int n);\nint pzn_b(int n)", ["pzn_b", "closing"]),                 # no `;` at the end
    ("int pzn_a(int n)\nint pzn_b(int n);", ["pzn_a", "pzn_b"]),                   # no `;` between two
    ("int pzn_a(int n, void (*cb)(int));", ["pzn_a"]),
    ("int pzn_a(int n); int pzn_a(float x);", ["pzn_a", "twice"]),
    ("enum { PZN_A = 1, PZN_B };", ["PZN_B"]),
    ("struct pzn_s { int a; };", ["pzn_s"]),
])
def test_parser_fails_closed(text, names):
    from puzzlenet_amd import _lib
    with pytest.raises(_lib.PznError) as e:
        _lib.parse_header(text, "some/dir/small.h")
    assert "some/dir/small.h" in str(e.value) and all(n in str(e.value) for n in names), str(e.value)


def test_missing_header_is_an_error(tmp_path):
    from puzzlenet_amd import _lib
    with pytest.raises(_lib.PznError, match="nowhere.h"):
        _lib.read_header(str(tmp_path / "nowhere.h"))
    assert os.path.samefile(_lib.HEADER_PATH, os.path.join(ROOT, "include", "pzn.h"))


# Library call sites whose argument count cannot be read off the source: the entry point's name is completed at run time (the
# "_f32" / "_f64" suffix) or the arguments are starred.  (file, entry point as written); the list may shrink, never grow.
_UNCOUNTED = [
    ("puzzlenet_amd/ops.py", "pzn_emd_approxmatch_"),
    ("puzzlenet_amd/ops.py", "pzn_emd_matchcost_"),
    ("puzzlenet_amd/ops.py", "pzn_emd_matchcost_grad_"),
    ("puzzlenet_amd/ops.py", "pzn_attn_fused_prep_weights_n"),
    ("puzzlenet_amd/ops.py", "pzn_attn_fused_proj"),
    ("tests/test_gpu_x3_exact.py", "pzn_attn_fused_wgrads"),
    ("tests/test_gpu_dense.py", "pzn_attn_fused_wgrads"),
    ("tests/test_gpu_fracture.py", "pzn_fracture_f32"),
    ("tests/test_gpu_fracture.py", "pzn_fracture_f32"),
]


def _call_sites():
    """Every `_call("pzn_...", ...)`, `_lib.call("pzn_...", ...)` and `<x>.pzn_...(...)` of the package, bench.py, tools/ and
    tests/ -> (file, line, entry point as written, name is a literal, arguments are starred, arguments that are not)."""
    import ast
    import glob
    files = (glob.glob(os.path.join(ROOT, "puzzlenet_amd", "**", "*.py"), recursive=True) + [os.path.join(ROOT, "bench.py")]
             + glob.glob(os.path.join(ROOT, "tools", "*.py")) + glob.glob(os.path.join(ROOT, "tests", "*.py")))
    for path in sorted(files):
        for node in ast.walk(ast.parse(open(path).read(), path)):
            if not isinstance(node, ast.Call) or not isinstance(node.func, (ast.Attribute, ast.Name)):
                continue
            fn = node.func.attr if isinstance(node.func, ast.Attribute) else node.func.id
            if fn.startswith("pzn_"):
                name, literal, args = fn, True, node.args
            elif fn in ("_call", "call") and node.args:
                written = [c.value for c in ast.walk(node.args[0])
                           if isinstance(c, ast.Constant) and isinstance(c.value, str) and c.value.startswith("pzn_")]
                if not written:
                    continue                                    # (a wrapper that passes its own `name` on)
                name, literal, args = written[0], isinstance(node.args[0], ast.Constant), node.args[1:]
            else:
                continue
            plain = [a for a in args if not isinstance(a, ast.Starred)]
            yield os.path.relpath(path, ROOT).replace(os.sep, "/"), node.lineno, name, literal, len(plain) < len(args), len(plain)


def test_every_call_site_passes_the_declared_number_of_arguments():
    """ctypes checks the count only when the call runs, on a GPU, on the path a test's shape happens to take."""
    from puzzlenet_amd import _lib
    sites = list(_call_sites())
    assert len(sites) > 200
    wrong, uncounted = [], []
    for path, line, name, literal, starred, got in sites:
        if literal:
            assert name in _lib.SIGNATURES, f"{path}:{line}: {name} is not declared in include/pzn.h"
            wants = {name: len(_lib.SIGNATURES[name][1])}
        else:                                                   # a prefix: every entry point one more word makes of it
            wants = {n: len(a) for n, (_, a) in _lib.SIGNATURES.items() if n.startswith(name) and "_" not in n[len(name):]}
            assert wants, f"{path}:{line}: no entry point of include/pzn.h is {name} + a suffix"
        if not literal or starred:
            uncounted.append((path, name))
        for n, want in wants.items():
            if (got > want) if starred else (got != want):
                wrong.append(f"{path}:{line}: {n} got {got}{' + starred' if starred else ''}, want {want}")
    assert not wrong, "\n".join(wrong)
    allowed = list(_UNCOUNTED)
    for site in uncounted:
        assert site in allowed, f"a call site whose arguments cannot be counted, beyond the listed ones: {site}"
        allowed.remove(site)


def test_no_hidden_symbols_leak(lib_path):
    import subprocess
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib_path]).decode()
    exported = [l.split()[-1] for l in out.splitlines() if " T " in l]
    ours = [s for s in exported if not s.startswith("_")]
    assert sorted(ours) == _declared()


def test_cpu_tensor_is_rejected_loudly():
    import torch
    from puzzlenet_amd import _lib, ops
    with pytest.raises(_lib.PznError):
        ops.knn(torch.zeros(1, 8, 3), torch.zeros(1, 2, 3), 2)


def test_product_does_not_import_oracle():
    """The product package must never route through the CPU oracle."""
    pkg = os.path.join(ROOT, "puzzlenet_amd")
    bad = []
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dp, f)).read()
                if re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M) or "pzn_oracle" in txt:
                    bad.append(f)
    assert not bad, bad


def test_integration_md_names_every_exported_symbol():
    """INTEGRATION.md is the index a maintainer binds from: every entry point include/pzn.h declares appears there (as its full
    name, inside a `pzn_x_{a,b}_f32` brace group, or as a ` / suffix` alternative of a named one)."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "pzn.h")).read()
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    syms = set(re.findall(r"\b(pzn_[a-z0-9_]+)\s*\(", header))
    names = set(re.findall(r"pzn_[a-z0-9_]+", doc))
    for m in re.finditer(r"(pzn_[a-z0-9_]*)\{([^}]*)\}([a-z0-9_]*)", doc):
        names.update(m.group(1) + alt.strip() + m.group(3) for alt in m.group(2).split(","))
    for m in re.finditer(r"(pzn_[a-z0-9_]+)((?:\s*/\s*_?[a-z0-9_]+)+)", doc):
        toks = m.group(1).split("_")
        for alt in (q.strip().lstrip("_") for q in m.group(2).split("/") if q.strip()):
            names.update("_".join(toks[:k]) + "_" + alt for k in range(1, len(toks)))
    missing = sorted(syms - names)
    assert not missing, f"entry points of include/pzn.h that INTEGRATION.md does not name: {missing}"
