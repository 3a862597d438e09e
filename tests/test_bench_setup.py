"""bench.py's set-up: the threaded weight fill gives the bits of synthetic.fill_module_, and the legs of --full refuse to run without it
(no GPU, no model work beyond a tiny model)."""
import importlib.util
import os
import subprocess
import sys

import pytest
import torch

import tiny

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location('bench_under_test', os.path.join(ROOT, 'bench.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)                  # top level defines functions / constants only
    return m


def test_threaded_fill_equals_fill_module():
    b = _bench()
    for variant in ('v1', 'v2'):
        ref = tiny.build(tiny.hip_ns(), variant, seed=1).state_dict()          # fill_module_(model, seed=1)
        for empty in (False, True):
            model = tiny.build(tiny.hip_ns(), variant, seed=5)                  # other weights, then the threaded fill over them
            if empty:
                model.to_empty(device='cpu')                                     # as bench.py does on the GPU: nothing kept from before
            got = b.fill_weights(model, 1, 4).state_dict()
            assert list(got) == list(ref)
            for k in ref:
                assert torch.equal(got[k], ref[k]), (variant, empty, k)


def test_fill_refuses_to_leave_a_tensor_unfilled():
    b = _bench()
    model = tiny.build(tiny.hip_ns(), 'v1')
    model.register_buffer('counter', torch.zeros(3, dtype=torch.int64))          # not floating: the fill would leave it as it is
    with pytest.raises(RuntimeError, match='counter'):
        b.fill_weights(model, 1, 2)


def test_full_legs_need_full():
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    for flag in ('--cpu-baseline-c2', '--parity-c4', '--parity-c5'):
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), flag], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and '--full' in r.stderr, (flag, r.returncode, r.stderr[-500:])
        assert r.stdout == ''
