"""The host half of the binding's operand check (hip._check_operand: dtype, element count or shape, layout, the extent of a row view) on CPU tensors,
and the structural property that `python -O` cannot remove a check: no `assert` statement anywhere in hip.py."""
import ast
import os

import pytest
import torch

from panst3r_amd import hip

F32, I32 = torch.float32, torch.int32


def ok(t, dtypes, n, **kw):
    hip._check_operand('some_wrapper', 'an_operand', t, dtypes, n, **kw)


def refused(t, dtypes, n, needle, **kw):
    with pytest.raises(RuntimeError) as e:
        ok(t, dtypes, n, **kw)
    msg = str(e.value)
    assert 'some_wrapper' in msg and 'an_operand' in msg and needle in msg, msg


def test_exact_and_at_least_counts():
    t = torch.zeros(12)
    ok(t, F32, 12)
    ok(t, (I32, F32), 12)
    refused(t, F32, 11, 'must hold 11 elements, got 12')             # an equality stays an equality: a larger buffer is not the one the contract names
    ok(t, F32, 11, at_least=True)
    ok(t, F32, 12, at_least=True)
    ok(torch.zeros(4, 3), F32, 12)
    ok(torch.zeros(0), F32, 0)
    ok(torch.zeros(5), F32, 0, at_least=True)


def test_one_element_short_is_refused_in_both_modes():
    t = torch.zeros(11)
    refused(t, F32, 12, 'must hold 12 elements, got 11')
    refused(t, F32, 12, 'must hold at least 12 elements, got 11', at_least=True)


def test_shapes():
    t = torch.zeros(4, 3)
    ok(t, F32, (4, 3))
    ok(t, F32, (-1, 3))
    refused(t, F32, (3, 3), 'shape')
    refused(t, F32, (-1, 4), 'shape')
    refused(t, F32, (12,), 'shape')
    refused(torch.zeros(12), F32, (-1, 3), 'shape')


def test_wrong_dtype():
    refused(torch.zeros(12, dtype=torch.float64), F32, 12, 'dtype')
    refused(torch.zeros(12, dtype=torch.int64), (I32, F32), 12, 'dtype')


def test_views_that_are_not_dense():
    refused(torch.zeros(3, 4).t(), F32, 12, 'contiguous')              # a transposed view of the right element count
    refused(torch.zeros(24)[::2], F32, 12, 'contiguous')               # a strided slice of the right element count
    refused(torch.zeros(4, 6)[:, :3], F32, 12, 'contiguous')
    ok(torch.zeros(24)[6:18], F32, 12)                                 # a dense slice is a dense buffer
    ok(torch.zeros(4, 6)[:, :3], F32, (4, 3), layout='rows')           # the retrieval operands: rows at a leading dimension
    refused(torch.zeros(3, 4).t(), F32, (4, 3), 'row-major', layout='rows')
    refused(torch.zeros(12), F32, 12, 'row-major', layout='rows')
    ok(torch.zeros(24)[::2], F32, 12, layout='any')


def rows_ok(t, rows, cols, **kw):
    ok(t, F32, (rows, cols), at_least=True, layout='rows', **kw)


def rows_refused(t, rows, cols, needle, **kw):
    refused(t, F32, (rows, cols), needle, at_least=True, layout='rows', **kw)


def test_row_views():
    """the host half of _Operands.rows: at least rows x cols at a leading dimension that keeps the rows apart"""
    pad = torch.zeros(4, 6)[:, :3]
    rows_ok(pad, 4, 3)                                                  # a padded view: leading dimension 6 over 3 columns
    rows_ok(pad, 3, 2)                                                  # more than asked for
    rows_ok(pad, -1, -1)                                                # its own extent
    rows_ok(pad, 0, 0)
    rows_refused(pad, 5, 3, 'shape')                                    # one row short
    rows_refused(pad, 4, 4, 'shape')                                    # one column narrow
    rows_refused(torch.zeros(3, 4).t(), 4, 3, 'row-major')              # a transposed view
    rows_refused(torch.zeros(12), 4, 3, 'shape')                        # a 1-D tensor
    rows_refused(torch.zeros(4, 3, 1), 4, 3, 'shape')
    rows_refused(torch.zeros(24).as_strided((4, 3), (2, 1)), 4, 3, 'leading dimension')        # rows that overlap
    rows_refused(torch.zeros(4, 1).expand(4, 3), 4, 3, 'row-major')
    for ld in (0, 1, 2, 7):                                             # ONE row: any stride
        rows_ok(torch.zeros(24).as_strided((1, 3), (ld, 1)), 1, 3)
    rows_ok(torch.zeros(24).as_strided((4, 3), (2, 1)), 1, 3)           # ... also the first row of a view whose further rows overlap
    refused(pad.double(), F32, (4, 3), 'dtype', at_least=True, layout='rows')
    ok(None, F32, (4, 3), at_least=True, layout='rows', optional=True)
    refused(None, F32, (4, 3), 'torch tensor', at_least=True, layout='rows')


def test_row_views_that_the_kernel_fills_up_to_the_leading_dimension():
    pad = torch.zeros(4, 6)[:, :3]                                      # the last row's padding reaches past the view, not past the storage
    rows_ok(pad, 4, 3, fill=True)
    cut = torch.zeros(23).as_strided((4, 3), (6, 1))                    # the same view of a buffer cut by one element
    rows_ok(cut, 4, 3)
    rows_refused(cut, 4, 3, 'storage', fill=True)
    rows_ok(cut, 3, 3, fill=True)                                       # fewer rows filled: inside again
    rows_ok(torch.zeros(30)[6:].as_strided((4, 3), (6, 1)), 4, 3, fill=True)
    rows_refused(torch.zeros(30)[7:].as_strided((4, 3), (6, 1)), 4, 3, 'storage', fill=True)   # the storage offset counts
    rows_refused(cut, -1, -1, 'storage', fill=True)


def test_cpu_row_view_is_refused_by_the_device_half():
    b = hip._Operands('some_wrapper')
    assert b.rows('an_operand', None, F32, 4, 3, optional=True) == (None, 0)
    with pytest.raises(RuntimeError, match='some_wrapper: an_operand .*shape'):
        b.rows('an_operand', torch.zeros(3, 3), F32, 4, 3)
    with pytest.raises(RuntimeError, match='some_wrapper: an_operand .*no CPU fallback'):
        b.rows('an_operand', torch.zeros(4, 6)[:, :3], F32, 4, 3)


def test_not_a_tensor():
    import numpy as np
    for t in (np.zeros(12, np.float32), [0.0] * 12, 12, 'x'):
        refused(t, F32, 12, 'torch tensor')


def test_none_passes_only_where_optional():
    ok(None, F32, 12, optional=True)
    ok(None, F32, (4, 3), optional=True)
    refused(None, F32, 12, 'torch tensor')
    refused(None, F32, 12, 'torch tensor', at_least=True)
    refused(torch.zeros(11), F32, 12, 'must hold', optional=True)       # an optional operand that is given is held to its contract


def test_cpu_tensor_is_refused_by_the_device_half():
    b = hip._Operands('some_wrapper')
    with pytest.raises(RuntimeError, match='some_wrapper: an_operand .*no CPU fallback'):
        b('an_operand', torch.zeros(12), F32, 12)
    assert b('an_operand', None, F32, 12, optional=True) is None
    with pytest.raises(RuntimeError, match='some_wrapper: a scene without quads'):
        b.require(False, 'a scene without quads')


# ---- the `python -O` property
def _calls(fn):
    return {n.func.id for n in ast.walk(fn) if isinstance(n, ast.Call) and isinstance(n.func, ast.Name)} | \
           {n.func.attr for n in ast.walk(fn) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute)}


def test_no_assert_anywhere_in_the_binding():
    path = os.path.join(os.path.dirname(os.path.abspath(hip.__file__)), 'hip.py')
    tree = ast.parse(open(path).read())
    fns = {}
    for node in ast.walk(tree):
        if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)):
            fns.setdefault(node.name, node)
    assert len(fns) > 200, len(fns)
    # the parse is not empty: it finds the launching entry points of both halves - those that call _call, or call (by name) a function that does
    reach = {name for name, fn in fns.items() if '_call' in _calls(fn)}
    grew = True
    while grew:
        more = {name for name, fn in fns.items() if name not in reach and _calls(fn) & reach}
        grew, reach = bool(more), reach | more
    assert len(reach) >= 100 and {'pp_finalize', 'icp_step', 'depth_errors', 'mesh_area_count', 'layernorm', 'gemm', 'attention', 'patch_rows'} <= reach, sorted(reach)
    bad = [a.lineno for a in ast.walk(tree) if isinstance(a, ast.Assert)]
    assert not bad, 'assert statements that python -O removes, at lines %s' % bad
