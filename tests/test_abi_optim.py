"""CPU: include/mla_hip_optim.h, the sibling of include/mla_hip.h (entry points added after the first header's symbol set was pinned
by test_abi.py), is treated like the first -- every symbol it declares is exported, hip.lib() hands its functions out with the
derived ctypes objects, and no name is declared in both headers (no compute calls)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols(name):
    txt = open(os.path.join(ROOT, "include", name)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(mla_[a-z0-9_]+)\s*\(", txt)) - {"mla_stream_t"})


def test_library_exports_every_symbol_of_the_sibling_header():
    import __graft_entry__ as g
    g.build()
    from mla_amd import hip
    lib = ctypes.CDLL(hip._LIB_PATH)
    syms = _header_symbols("mla_hip_optim.h")
    assert "mla_adamw_m16_step" in syms
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, f"declared in include/mla_hip_optim.h but not exported: {missing}"
    # the derived table and this file's looser regex agree on the symbol set: the parser skipped nothing
    assert set(hip._OPTIM_SIGNATURES) == set(hip._OPTIM_RESTYPES) == set(syms), set(hip._OPTIM_SIGNATURES) ^ set(syms)
    # every function lib() hands out carries the derived objects, none is left on ctypes' defaults
    L = hip.lib()
    for s in syms:
        fn = getattr(L, s)
        assert fn.restype is hip._OPTIM_RESTYPES[s] and list(fn.argtypes) == hip._OPTIM_SIGNATURES[s], s
    # no name is declared in both headers; the first header's tables keep describing it alone
    both = set(syms) & set(_header_symbols("mla_hip.h"))
    assert not both, both
    assert not set(syms) & set(hip._SIGNATURES) and not set(syms) & set(hip.exported_symbols())


def test_m16_signature_as_derived():
    from ctypes import c_float, c_int, c_longlong, c_ulonglong, c_void_p
    from mla_amd import hip
    P, F, LL = c_void_p, c_float, c_longlong
    assert hip._OPTIM_RESTYPES["mla_adamw_m16_step"] is c_int
    assert hip._OPTIM_SIGNATURES["mla_adamw_m16_step"] == [P, P, P, P, P, P, LL, LL, F, F, F, F, F, c_int, P, F, F, c_ulonglong, LL, P]


def test_build_force_includes_both_headers():
    """build.sh shows both headers to the compiler next to every definition and rebuilds an object older than either."""
    sh = open(os.path.join(ROOT, "mla_amd", "csrc", "build.sh")).read()
    compiles = [ln for ln in sh.splitlines() if "$HIPCC $FLAGS" in ln]
    assert compiles and all('-include "$HDR" -include "$HDR2"' in ln for ln in compiles), compiles
    assert 'HDR2="$HERE/../../include/mla_hip_optim.h"' in sh and '[ "$HDR2" -nt "$BUILD/$f.o" ]' in sh


def test_m16_argument_validation_on_the_host():
    """Argument validation happens before any launch -> safe without a GPU."""
    from mla_amd import hip
    L = hip.lib()
    P = ctypes.c_void_p(256)
    hy = (2e-5, 0.9, 0.999, 1e-8, 0.01)

    def call(p=P, g=P, m=P, v=P, ema=None, n=64, n_decay=64, step=1, d=0.0, omd=0.0, base=0):
        return L.mla_adamw_m16_step(p, g, m, v, ema, None, n, n_decay, *hy, step, None, d, omd, 7, base, None)

    for kw in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(n=-1, n_decay=0), dict(step=0), dict(n_decay=-1), dict(n_decay=65),
               dict(base=-1), dict(ema=P, d=1.5, omd=0.0), dict(ema=P, d=0.5, omd=-0.5), dict(ema=P, d=float("nan"), omd=0.5),
               dict(ema=P, d=0.5, omd=float("nan"))):
        assert call(**kw) == -1, kw
        assert b"mla_adamw_m16_step" in L.mla_last_error()
    assert call(n=0, n_decay=0) == 0                    # a valid no-op
