"""The host half of the binding's operand check (hip._check_operand: dtype, element count or shape, layout) on CPU tensors, and the structural
property that `python -O` cannot remove a check: no `assert` statement in any engine wrapper of hip.py that reaches `_call`."""
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
FIRST_ENGINE_WRAPPER = 'pp_scores'      # the in-scope half of hip.py starts here and runs to the end of the file


def _calls(fn):
    return {n.func.id for n in ast.walk(fn) if isinstance(n, ast.Call) and isinstance(n.func, ast.Name)} | \
           {n.func.attr for n in ast.walk(fn) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute)}


def test_no_assert_in_an_engine_wrapper_that_reaches_call():
    path = os.path.join(os.path.dirname(os.path.abspath(hip.__file__)), 'hip.py')
    tree = ast.parse(open(path).read())
    fns = {}
    for node in ast.walk(tree):
        if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)):
            fns.setdefault(node.name, node)
    start = fns[FIRST_ENGINE_WRAPPER].lineno
    engine = {name: fn for name, fn in fns.items() if fn.lineno >= start}
    assert len(engine) > 100, len(engine)
    # reaches _call: calls it, or calls (by name) an in-scope function that does
    reach = {name for name, fn in engine.items() if '_call' in _calls(fn)}
    grew = True
    while grew:
        more = {name for name, fn in engine.items() if name not in reach and _calls(fn) & reach}
        grew, reach = bool(more), reach | more
    assert len(reach) >= 70 and {'pp_finalize', 'icp_step', 'depth_errors', 'mesh_area_count'} <= reach, sorted(reach)      # the launching entry points
    # ... and everything such a wrapper calls on the way: its helpers in that half, and the check itself
    helpers = {h for name in reach for h in _calls(engine[name]) if h in engine} | reach
    checked = [engine[n] for n in helpers] + [fns['_check_operand']] + \
              [n for n in ast.walk(tree) if isinstance(n, ast.ClassDef) and n.name in ('_Operands', 'DepthTable')]
    bad = [(getattr(fn, 'name', '?'), a.lineno) for fn in checked for a in ast.walk(fn) if isinstance(a, ast.Assert)]
    assert not bad, 'assert statements that python -O removes: %s' % bad
    # the two refusals no tensor carries are statements too
    for name in ('_view_table', 'consist_view_table', 'depth_table'):
        assert not [a for a in ast.walk(engine[name]) if isinstance(a, ast.Assert)], name
