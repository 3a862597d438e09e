"""The C-ABI library loads and exports every symbol include/panst3r_hip.h declares, and the ctypes binding declares the types the header does
(no compute calls: no GPU here)."""
import ctypes
import os
import re

import abi_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALAR = {'int': ctypes.c_int, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'uint64_t': ctypes.c_uint64, 'float': ctypes.c_float,
          'double': ctypes.c_double}
assert set(SCALAR) == set(abi_header.SCALARS)


def declared_symbols():
    return sorted(p[0] for p in abi_header.prototypes())


def test_library_builds_and_exports_all_symbols():
    from panst3r_amd.build import build
    from panst3r_amd import hip
    path = build(verbose=False)
    lib = ctypes.CDLL(path)
    syms = declared_symbols()
    assert len(syms) >= 15
    for s in syms:
        assert hasattr(lib, s), s
    assert set(syms) == set(hip.EXPORTS) == set(hip.SIGNATURES) and len(hip.EXPORTS) == len(syms)
    lib.pst_abi_version.restype = ctypes.c_int
    assert lib.pst_abi_version() == hip.ABI_VERSION == abi_header.defines()['PST_ABI_VERSION']


def _ctype(t, by_reference):
    """what the binding must declare for the header's type `t`: the scalar itself; for a pointer, a pointer to the ctypes struct where the host passes
    that struct by reference, else an address (device memory, the stream), and `const char*` only as a returned string"""
    if t in by_reference:
        return ctypes.POINTER(by_reference[t])
    return ctypes.c_void_p if t.endswith('*') else SCALAR[t]


def test_signatures_match_header():
    """restype and argtypes of every entry point, as hip.lib() declares them on the built library, are the header's prototype"""
    from panst3r_amd.build import build
    from panst3r_amd import hip
    build(verbose=False)
    lib = hip.lib()
    protos = abi_header.prototypes()
    assert len(protos) == len(hip.SIGNATURES) and {p[0] for p in protos} == set(hip.SIGNATURES)
    by_ref = {'pst_gemm_params*': hip.GemmParams, 'pst_attn_params*': hip.AttnParams}      # (pst_cloud_view* is a table in device memory: an address)
    for name, ret, params in protos:
        fn = getattr(lib, name)
        assert ret in ('int', 'int64_t', 'char*'), (name, ret)
        assert fn.restype is (ctypes.c_char_p if ret == 'char*' else SCALAR[ret]), '%s returns %s, declared %s' % (name, ret, fn.restype)
        assert 'char*' not in params, name
        want = [_ctype(t, by_ref) for t in params]
        got = list(fn.argtypes)
        assert len(got) == len(want), '%s takes %d arguments, declared %d' % (name, len(want), len(got))
        for i, (g, w, t) in enumerate(zip(got, want, params)):
            assert g is w, '%s argument %d is %s, declared %s' % (name, i, t, g.__name__)


def test_struct_layouts_match_header():
    """ctypes mirrors of pst_gemm_params / pst_attn_params / pst_cloud_view have the fields of the header: names, types and array lengths, in order."""
    from panst3r_amd import hip
    structs = abi_header.structs()
    mirrors = {'pst_gemm_params': hip.GemmParams, 'pst_attn_params': hip.AttnParams, 'pst_cloud_view': hip.CloudView}
    assert set(structs) == set(mirrors)
    for cname, ctype in mirrors.items():
        fields = structs[cname]
        assert [f[0] for f in fields] == [f[0] for f in ctype._fields_], (cname, [f[0] for f in fields])
        for (fname, typ, n), (_, got) in zip(fields, ctype._fields_):
            want = _ctype(typ, {})
            want = want * n if n else want          # (ctypes caches array types: c_float * 12 is one object)
            assert got is want, '%s.%s is %s%s, declared %s' % (cname, fname, typ, '[%d]' % n if n else '', got.__name__)
    assert ctypes.sizeof(hip.CloudView) == 104


def test_product_refuses_cpu_tensors():
    import pytest
    import torch
    from panst3r_amd import hip
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hip.gemm(torch.zeros(64, 64, dtype=torch.bfloat16), torch.zeros(64, 64, dtype=torch.bfloat16), torch.zeros(64, 64))


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, 'panst3r_amd')
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith('.py'):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r'^\s*(from|import)\s+oracle\b', src, flags=re.M), f


def test_only_the_allowed_places_import_the_oracle():
    """oracle/ is test infrastructure: besides tests/ only __graft_entry__.smoke() and bench.py's cpu_baseline leg may import it.
    tools/ must not (oracle-checking diagnostics live in tests/diag/), and bench.py only inside cpu_baseline()."""
    pat = re.compile(r'^(\s*)(from|import)\s+oracle\b', flags=re.M)
    for f in os.listdir(os.path.join(ROOT, 'tools')):
        if f.endswith('.py'):
            assert not pat.search(open(os.path.join(ROOT, 'tools', f)).read()), f
    src = open(os.path.join(ROOT, 'bench.py')).read()
    hits = [m for m in pat.finditer(src)]
    assert hits and all(len(m.group(1)) > 0 for m in hits)                      # function-level imports only
    # ... and only inside the functions of the cpu_baseline leg (cpu_baseline, cpu_c1): find the enclosing def of every import
    for m in hits:
        defs = [d for d in re.finditer(r'^def (\w+)\(', src[:m.start()], flags=re.M)]
        assert defs and defs[-1].group(1).startswith('cpu_'), defs[-1].group(1) if defs else None
    # (__graft_entry__.build() import-checks the Python oracle as its "build the checker" step, which is allowed; smoke() uses it)


def test_diag_and_tool_scripts_compile():
    """tests/diag, tools/ and the golden generator only run by hand (GPU box / build container): keep them at least syntactically valid."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, 'tests', 'diag', '*.py')) + glob.glob(os.path.join(ROOT, 'tools', '*.py')) +
                   [os.path.join(ROOT, 'tests', 'golden', 'make_golden.py'), os.path.join(ROOT, 'bench.py'), os.path.join(ROOT, '__graft_entry__.py')])
    assert len(files) >= 12
    for f in files:
        compile(open(f).read(), f, 'exec')            # syntax only: nothing is executed or written
