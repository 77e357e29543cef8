"""CPU: the C-ABI library loads and exports every symbol include/misplat.h declares, the ctypes
mirror of misplat_params matches the C layout, and the product path fails loudly (no fallback,
no route through oracle/).  No compute calls: there is no GPU here."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "misplat.h")


ARG_KIND = {"int": "i", "int32_t": "i", "int64_t": "q", "float": "f", "double": "d", "uint32_t": "u", "size_t": "Q",
            "misplat_stream_t": "s"}
RET_KIND = {"int": "i", "int64_t": "q", "void": "v", "const char*": "z", "misplat_graph_cache*": "p"}


def declared_signatures():
    """name -> signature string (the format of _lib.SYMBOLS) of every prototype of the header."""
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    sigs = {}
    for ret, name, args in re.findall(r"^\s*((?:const\s+)?\w+(?:\s*\*)?)\s*(misplat_\w+)\s*\(([^()]*)\)\s*;", text, flags=re.M):
        kinds = ""
        for a in ([] if args.strip() in ("", "void") else args.split(",")):
            # a pointer is a pointer whatever it points to; a value is named by the first word after any const
            kinds += "p" if "*" in a or "[" in a else ARG_KIND[re.sub(r"\bconst\b", "", a).split()[0]]
        assert name not in sigs, name
        sigs[name] = (RET_KIND[re.sub(r"\s*\*", "*", " ".join(ret.split()))] + " " + kinds).strip()
    return sigs


def declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(misplat_[a-z0-9_]+)\s*\(", text)))


def test_header_and_binding_agree():
    """Every prototype of the header has its signature in _lib.SYMBOLS and nothing else is there: the return kind, every
    argument's kind, and the stream exactly where the header says misplat_stream_t."""
    from collab_splats_amd import _lib
    sigs = declared_signatures()
    assert sorted(sigs) == declared_symbols()              # the prototype pattern missed no name the header calls
    assert sorted(sigs) == sorted(_lib.SYMBOLS)
    wrong = {n: (s, _lib.SYMBOLS[n]) for n, s in sigs.items() if s != _lib.SYMBOLS[n]}
    assert not wrong, wrong
    assert all(set(s[2:]) <= set(_lib._ARG) and s[0] in _lib._RET for s in _lib.SYMBOLS.values())


def test_argument_count_and_kind_are_checked(built_lib):
    from collab_splats_amd import _lib
    size = _lib.load().misplat_mcmc_sample_workspace_bytes
    with pytest.raises(_lib.MisplatError, match="0 arguments passed, the C ABI takes 1"):
        size()
    with pytest.raises(_lib.MisplatError, match="2 arguments passed, the C ABI takes 1"):
        size(4, 4)
    with pytest.raises(C.ArgumentError):
        size(4.0)


def test_sixty_four_bit_arguments_and_returns_keep_their_width(built_lib):
    """Host-only size functions: csrc/mcmc.hip admits 1 .. 2^31 - 1 rows and carves more than 8 bytes a row."""
    from collab_splats_amd import _lib
    size = _lib.load().misplat_mcmc_sample_workspace_bytes
    assert size(2 ** 32 + 5) == -1                         # (a 32-bit pass would see 5 and return a size)
    assert size(2 ** 31 - 1) > 2 ** 31
    for n in (1, 1000, 2 ** 31 - 1, 2 ** 32 + 5):
        assert size(n) == size(C.c_int64(n))


def test_library_exports_every_declared_symbol(built_lib):
    from collab_splats_amd import _lib
    lib = _lib.load()
    for name in declared_symbols():
        assert hasattr(lib, name), name
    assert lib.misplat_version().decode().endswith("gfx950")
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (misplat_\w+)", out))
    assert exported == set(declared_symbols())          # nothing else leaks out of the C ABI


def test_library_contains_gfx950_code_object(built_lib):
    data = open(built_lib, "rb").read()
    assert b"gfx950" in data and b"blend_bwd_kernel" in data


def test_params_struct_layout_matches_c(built_lib):
    from collab_splats_amd._lib import Params
    fields = [f[0] for f in Params._fields_]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"misplat.h\"\nint main(){printf(\"%zu\\n\", sizeof(misplat_params));\n"
    src += "".join(f'printf("%zu\\n", offsetof(misplat_params, {f}));\n' for f in fields) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        vals = [int(x) for x in subprocess.check_output([exe]).split()]
    assert vals[0] == C.sizeof(Params)
    assert vals[1:] == [getattr(Params, f).offset for f in fields]


@pytest.mark.parametrize("cname,pyname", [("misplat_raster_args", "RasterArgs"), ("misplat_raster_bwd_args", "RasterBwdArgs")])
def test_raster_args_struct_layout_matches_c(built_lib, cname, pyname):
    from collab_splats_amd import _lib
    RasterArgs = getattr(_lib, pyname)
    fields = [f[0] for f in RasterArgs._fields_]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"misplat.h\"\nint main(){printf(\"%zu\\n\", sizeof(" + cname + "));\n"
    src += "".join(f'printf("%zu\\n", offsetof({cname}, {f}));\n' for f in fields) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        vals = [int(x) for x in subprocess.check_output([exe]).split()]
    assert vals[0] == C.sizeof(RasterArgs)
    assert vals[1:] == [getattr(RasterArgs, f).offset for f in fields]


def test_no_cpu_fallback():
    import collab_splats_amd as m
    z = torch.zeros
    with pytest.raises(m.MisplatError):
        m.rasterization(z(2, 3), z(2, 4), z(2, 3), z(2), z(2, 3), torch.eye(4)[None], torch.eye(3)[None], 8, 8)
    with pytest.raises(m.MisplatError):
        m.fully_fused_projection(z(2, 3), None, z(2, 4), z(2, 3), torch.eye(4)[None], torch.eye(3)[None], 8, 8)
    with pytest.raises(m.MisplatError):
        m.spherical_harmonics(0, z(2, 3), z(2, 1, 3))


def test_missing_library_fails_loudly(monkeypatch):
    from collab_splats_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libmisplat.so")
    with pytest.raises(_lib.MisplatError, match="no CPU fallback"):
        _lib.load()


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "collab_splats_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M), f
                assert "craster" not in text and "torch_oracle" not in text, f
    code = "import sys; import collab_splats_amd; assert not any(m.split('.')[0]=='oracle' for m in sys.modules)"
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


def test_argument_validation_matches_reference_errors():
    import collab_splats_amd as m
    z = torch.zeros
    args = (z(2, 3), z(2, 4), z(2, 3), z(2), z(2, 3), torch.eye(4)[None], torch.eye(3)[None], 8, 8)
    with pytest.raises(ValueError, match="rasterize_mode"):      # rade_gs_model.py:150-151
        m.rasterization(*args, rasterize_mode="fancy")
    with pytest.raises(ValueError, match="render_mode"):
        m.rasterization(*args, render_mode="XYZ")
    with pytest.raises(NotImplementedError):
        m.rasterization(*args, packed=True)
    with pytest.raises(AssertionError):
        m.rasterization(z(2, 3), z(3, 4), z(2, 3), z(2), z(2, 3), torch.eye(4)[None], torch.eye(3)[None], 8, 8)


def test_gsplat_alias_resolves_reference_imports():
    code = ("import collab_splats_amd as m; m.install_gsplat_alias();"
            "from gsplat.rendering import rasterization;"
            "from gsplat.strategy import DefaultStrategy;"
            "from gsplat.cuda._wrapper import fully_fused_projection, spherical_harmonics;"
            "assert rasterization is m.rasterization and DefaultStrategy().absgrad is False")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


def test_gsplat_alias_serves_nerfstudio_style_imports_and_names_what_is_missing():
    """nerfstudio's Splatfacto imports more of gsplat than the reference itself
    (``from gsplat.strategy import DefaultStrategy, MCMCStrategy``): those lines must resolve against the alias, and
    anything that is not built must say so instead of failing with a bare AttributeError."""
    import importlib
    import sys
    import collab_splats_amd
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "gsplat" or k.startswith("gsplat.")}
    try:
        collab_splats_amd.install_gsplat_alias()
        ns = {}
        exec("from gsplat.strategy import DefaultStrategy, MCMCStrategy\n"
             "from gsplat.rendering import rasterization\n"
             "from gsplat.cuda._wrapper import fully_fused_projection, spherical_harmonics\n"
             "from gsplat import rasterization as r2, DefaultStrategy as d2\n"
             "import gsplat", ns)
        assert ns["DefaultStrategy"] is collab_splats_amd.DefaultStrategy and ns["r2"] is collab_splats_amd.rasterization
        with pytest.raises(NotImplementedError):
            ns["MCMCStrategy"]()
        with pytest.raises(ImportError, match="not provided by collab_splats_amd"):
            exec("from gsplat import rasterization_2dgs", {})
        with pytest.raises(ImportError, match="not provided"):
            getattr(ns["gsplat"].cuda, "_backend")
    finally:
        for k in [k for k in sys.modules if k == "gsplat" or k.startswith("gsplat.")]:
            sys.modules.pop(k)
        sys.modules.update(saved)
