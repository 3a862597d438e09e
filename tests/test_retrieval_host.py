"""The checkpoint retriever's host side (panst3r_amd/model/retrieval.py): loader layouts, the parameter and key checks, and known-answer cases of
the float64 restatement (tests/retrieval_ref.py) that the GPU tests compare against.  No GPU needed."""
import numpy as np
import pytest
import torch

import retrieval_ref as R
from panst3r_amd.model.retrieval import RetrievalASMK, RetrievalSpecError


def small(**kw):
    kw.setdefault('k', 64)
    return R.make_dict(3, **kw)


@pytest.mark.parametrize('layout', ['dict', 'tensor', 'array'])
def test_loader_codebook_layouts(layout):
    ck = small(layout=layout)
    r = RetrievalASMK(ck)
    assert (r.k, r.D, r.d_in, r.nfeat) == (64, 128, 128, 40)
    assert torch.equal(r.centroids, torch.from_numpy(R.centroids_of(ck).astype(np.float32)))
    assert r.params == dict(ma_db=1, ma_q=5, alpha=3.0, tau=0.0)


def test_loader_reads_a_path(tmp_path):
    ck = small(hdims='96', prewhiten=True)
    f = tmp_path / 'retrieval.pth'
    torch.save(ck, str(f))
    r = RetrievalASMK(str(f))
    assert (r.k, r.D) == (64, 128) and [s[0] for s in r.stages] == ['white', 'proj']
    with pytest.raises(FileNotFoundError):
        RetrievalASMK(str(tmp_path / 'missing.pth'))


@pytest.mark.parametrize('hdims,pre,post,residual,d_out', [('', False, False, False, None), ('96', True, False, True, None), ('128_64', False, True, False, None),
                                                           ('', True, True, False, 96), ('96', True, True, False, 64)])
def test_loader_head_structures(hdims, pre, post, residual, d_out):
    ck = small(hdims=hdims, prewhiten=pre, postwhiten=post, residual=residual, d_out=d_out)
    r = RetrievalASMK(ck)
    assert r.D == R.centroids_of(ck).shape[1] == (d_out or 128) and r.d_in == 128
    kinds = (['white'] if pre else []) + (['proj'] if (hdims or residual or d_out) else []) + (['white'] if post else [])
    assert [s[0] for s in r.stages] == kinds


def test_defaults_when_params_are_absent():
    r = RetrievalASMK(small(params={}))
    assert r.params == dict(ma_db=1, ma_q=5, alpha=3.0, tau=0.0)


@pytest.mark.parametrize('path,value,match', [
    (('build_ivf', 'kernel', 'binary'), False, 'binary'),
    (('build_ivf', 'ivf', 'use_idf'), True, 'idf'),
    (('query_ivf', 'search', 'topk'), 10, 'top-k'),
    (('query_ivf', 'similarity', 'similarity_threshold'), -0.1, 'similarity_threshold'),
    (('query_ivf', 'similarity', 'alpha'), 0.0, 'alpha'),
    (('query_ivf', 'quantize', 'multiple_assignment'), 9, 'multiple_assignment'),
])
def test_unsupported_parameters_raise(path, value, match):
    params = {}
    d = params
    for p in path[:-1]:
        d = d.setdefault(p, {})
    d[path[-1]] = value
    with pytest.raises(RetrievalSpecError, match=match):
        RetrievalASMK(small(params=params))


def test_unsupported_head_and_codebook_raise():
    ck = small(d_out=48)                                    # D = 48: not a multiple of 32
    with pytest.raises(RetrievalSpecError, match='multiple of 32'):
        RetrievalASMK(ck)
    ck = small()
    ck['args'].featweights = 'gem'
    with pytest.raises(RetrievalSpecError, match='featweights'):
        RetrievalASMK(ck)
    ck = small()
    ck['asmk_codebook'] = {'weights': np.zeros((4, 128), np.float32), 'params': {}}
    with pytest.raises(RetrievalSpecError, match="'params', 'weights'"):
        RetrievalASMK(ck)
    ck = small()
    del ck['asmk_params']
    with pytest.raises(RetrievalSpecError, match='asmk_params'):
        RetrievalASMK(ck)


def test_mismatched_head_keys_raise():
    ck = small(hdims='96')
    ck['model']['projector.9.weight'] = torch.zeros(3, 3)
    with pytest.raises(RetrievalSpecError, match='unexpected keys projector.9.weight'):
        RetrievalASMK(ck)
    ck = small(hdims='96')
    del ck['model']['projector.1.bias']
    with pytest.raises(RetrievalSpecError, match='missing key projector.1.bias'):
        RetrievalASMK(ck)
    ck = small(hdims='96')
    ck['args'].hdims = '64'
    with pytest.raises(RetrievalSpecError, match='hdims'):
        RetrievalASMK(ck)
    ck = small(hdims='96', prewhiten=True)
    del ck['model']['prewhiten.p']
    with pytest.raises(RetrievalSpecError, match='prewhiten.p'):
        RetrievalASMK(ck)
    ck = small()
    ck['model']['postwhiten.m'] = torch.zeros(1, 64, dtype=torch.float64)
    ck['model']['postwhiten.p'] = torch.zeros(64, 64, dtype=torch.float64)
    with pytest.raises(RetrievalSpecError, match='outputs 64 dims, the codebook has 128'):
        RetrievalASMK(ck)
    ck = small()                                           # backbone.* keys are ignored
    ck['model']['backbone.enc_blocks.0.attn.qkv.weight'] = torch.zeros(2, 2)
    RetrievalASMK(ck)


# ---------------------------------------------------------------------------------------------------- restatement known answers
D = 32


def _basis(w):
    e = np.zeros(D)
    e[w] = 10.0
    return e


def _desc(w, signs, mag=0.1, second=None):
    """a descriptor at 10 e_w + residual with the given signs (second-nearest word steered by a larger residual on that axis)"""
    r = mag * np.asarray(signs, dtype=np.float64)
    if second is not None:
        r[second] = 0.5
    return _basis(w) + r


def test_restatement_known_answers():
    cent = np.stack([_basis(w) for w in range(3)])
    plus = np.ones(D)
    plus[[0, 1, 2]] = 1
    flip8 = plus.copy()
    flip8[8:16] = -1                                       # D / 4 of the signs flipped
    # view 0: one descriptor on word 0; view 1: the same signs on word 0, one on word 1; view 2: word 0 with D/4 signs flipped
    desc = np.stack([_desc(0, plus, second=1), _desc(0, plus, second=1), _desc(1, plus, second=2), _desc(0, flip8, second=2)])
    counts = [1, 2, 1]
    ids, dist = R.assign(desc, cent, 2)
    assert ids.tolist() == [[0, 1], [0, 1], [1, 2], [0, 2]]
    assert np.all(np.diff(dist, axis=1) >= 0)
    agg = R.aggregate(desc, cent, ids, counts, 1)
    assert [w for w, _ in agg[1]] == [0, 1]
    assert np.array_equal(agg[0][0][1] > 0, plus > 0) and np.array_equal(agg[2][0][1] > 0, flip8 > 0)
    S = R.scores(agg, agg, D, 3.0, 0.0)
    assert S[0, 1] == 1.0 and S[1, 0] == 1.0                # identical residual signs: kappa = 1
    assert S[0, 2] == 0.5 ** 3 and S[2, 0] == 0.5 ** 3      # D / 4 flipped bits: s = 0.5
    assert S[1, 1] == 2.0 and S[0, 0] == 1.0
    S = R.scores(agg, agg, D, 3.0, 0.6)                     # the flipped word is below tau
    assert S[0, 2] == 0.0 and S[0, 1] == 1.0
    # the fp32 emulation of the kernel gives the same exact values here
    words = [[w for w, _ in agg[v]] for v in range(3)]
    bits = [np.stack([s > 0 for _, s in agg[v]]) for v in range(3)]
    assert np.array_equal(R.scores_f32(words, bits, words, bits, D, 3.0, 0.0), R.scores(agg, agg, D, 3.0, 0.0).astype(np.float32))


def test_restatement_multiple_assignment_and_asymmetry():
    """query side with ma = 2: a descriptor also joins its second word, so S is not symmetric"""
    cent = np.stack([_basis(w) for w in range(3)])
    plus = np.ones(D)
    desc = np.stack([_desc(0, plus, second=1), _desc(1, plus, second=2)])
    ids, _ = R.assign(desc, cent, 2)
    q = R.aggregate(desc, cent, ids, [1, 1], 2)
    db = R.aggregate(desc, cent, ids, [1, 1], 1)
    S = R.scores(q, db, D, 3.0, 0.0)
    assert [w for w, _ in q[0]] == [0, 1] and [w for w, _ in db[1]] == [1]
    assert S[0, 1] != 0.0 and S[1, 0] == 0.0


def test_selection_ties_go_to_the_lower_token():
    ck = small(k=64, nfeat=2)
    x = np.zeros((4, 128))
    x[:, 0] = [1.0, 2.0, 2.0, 0.5]                          # identity head: rows 1 and 2 tie
    desc, counts, toks = R.descriptors(ck, [x])
    assert counts == [2] and toks[0].tolist() == [1, 2]
    ck = small(k=64, nfeat=10)                              # nfeat above T keeps every row
    assert R.descriptors(ck, [x])[1] == [4]
