"""SigLIP text tower on the GPU: parity with the reference's TextEncoder (reference-generated fixture) and with live transformers at full size, the tanh
GELU epilogue (gemm act 3), the token-id guard, and set_vocab / live mode end to end through PanSt3R (eager and captured graphs)."""
import pytest
import torch
import torch.nn.functional as F

import errbound as EB
import text_tiny as T

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def rel_rows(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm(dim=-1) / b.norm(dim=-1)).max().item()


@pytest.fixture(scope='module')
def fx():
    return T.fixture()


@pytest.fixture(scope='module')
def tiny_dir(fx, tmp_path_factory):
    return T.write_tower(fx, str(tmp_path_factory.mktemp('siglip_tiny')), tokenizer=True)


def test_fixture_parity(fx, tiny_dir):
    """set_vocab / forward of the reference's TextEncoder (fixture: its own code on transformers' SiglipTextModel, fp32 CPU) against the HIP tower.
    rel-L2 per class <= 1e-5 (exact fp32 products, different summation order); measured on an MI355X: 6.9e-7 (store and forward)."""
    from panst3r_amd.model.panoptic import TextEncoder
    from panst3r_amd.model.text import MODEL_CONFIGS
    te = TextEncoder('siglip')
    tw = te.load_text_model(tiny_dir)
    cls = fx['classes']
    enc = tw.tokenizer([MODEL_CONFIGS['siglip']['template'].format(c) for c in cls], return_tensors='pt', **MODEL_CONFIGS['siglip']['tokenizer_args'])
    assert torch.equal(enc['input_ids'].int(), fx['ids']) and 'attention_mask' in enc        # same tokens, and the key-padding mask is in play
    te.set_vocab(cls)
    assert list(te.class_embeddings) == cls
    store = torch.stack([te.class_embeddings[c] for c in cls])
    assert store.is_cuda and store.dtype == torch.float32
    assert rel_rows(store, fx['store']) <= 1e-5
    assert rel_rows(te(cls), fx['forward']) <= 1e-5
    te.change_mode(fixed_vocab=False)
    assert rel_rows(te(cls), fx['forward_live']) <= 1e-5
    assert rel_rows(te(cls[::-1]), fx['forward_live'].flip(0)) <= 1e-5


def _full_size(cls_model, cls_cfg, tmp, vocab=4096):
    torch.manual_seed(0)
    cfg = cls_cfg(vocab_size=vocab, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12, max_position_embeddings=64)
    m = cls_model(cfg).eval()
    m.save_pretrained(tmp)
    return m


def _tokens(vocab, B=32, L=64, seed=3):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, vocab, (B, L), generator=g)
    lens = torch.randint(4, L + 1, (B,), generator=g)
    lens[0], lens[1] = L, 1                                     # a row without padding and one with a single token
    am = (torch.arange(L)[None] < lens[:, None]).long()
    ids = torch.where(am.bool(), ids, torch.ones_like(ids))    # pad id 1 (SigLIP's </s>) behind the text
    return ids, am


@pytest.mark.parametrize('kind', ['siglip', 'siglip2'])
def test_full_size_parity_with_transformers(kind, tmp_path):
    """Base dimensions (768, 12 layers x 12 heads, 3072, 64 positions), seeded random init, save_pretrained -> the HIP loader.  32 sequences of 64 tokens
    against transformers' pooler_output (fp32, CPU): rel-L2 per row <= 1e-5, with the padding mask and (SigLIP) without it.  Measured on an MI355X:
    1.7e-6 masked, 1.3e-6 unmasked; the mask itself moves the reference rows by 1.37 (rel-L2)."""
    tr = pytest.importorskip('transformers')
    if kind == 'siglip':
        m = _full_size(tr.SiglipTextModel, tr.SiglipTextConfig, str(tmp_path))
    else:
        m = _full_size(tr.Siglip2TextModel, tr.Siglip2TextConfig, str(tmp_path))
    from panst3r_amd.model.text import load_siglip_tower
    tw = load_siglip_tower(str(tmp_path), tokenizer=False)
    ids, am = _tokens(4096)
    with torch.no_grad():
        ref_m = m(input_ids=ids, attention_mask=am).pooler_output
        ref_u = m(input_ids=ids).pooler_output
    assert rel_rows(ref_u, ref_m) > 1e-3                        # ignoring the mask cannot pass
    got_m = tw.embed(ids.to(DEV), am.to(DEV))
    assert got_m.shape == (32, 768)
    assert rel_rows(got_m, ref_m) <= 1e-5
    if kind == 'siglip':
        assert rel_rows(tw.embed(ids.to(DEV)), ref_u) <= 1e-5
        # a sequence length that is not a multiple of 8 (padded inside, masked keys), and the caller's precision context is left as it was
        from panst3r_amd import hip
        from panst3r_amd.model.common import precision, PREC
        with torch.no_grad():
            ref_s = m(input_ids=ids[:5, :37], attention_mask=am[:5, :37]).pooler_output
        with precision('fp16'):
            got_s = tw.embed(ids[:5, :37].to(DEV), am[:5, :37].to(DEV))
            assert PREC.dtype == torch.float16 and hip.X3 is True
        assert rel_rows(got_s, ref_s) <= 1e-5


def test_gemm_act3_is_tanh_gelu():
    from panst3r_amd import hip
    from panst3r_amd.model.common import precision
    g = torch.Generator(device=DEV).manual_seed(1)
    a = torch.randn(300, 256, device=DEV, generator=g)
    w = torch.randn(512, 256, device=DEV, generator=g) * 0.15
    b = torch.randn(512, device=DEV, generator=g)
    with precision('fp32_exact'):
        pre = hip.gemm(a, w, torch.empty(300, 512, device=DEV), bias=b)
        out = hip.gemm(a, w, torch.empty(300, 512, device=DEV), bias=b, act='gelu_tanh')
        erf = hip.gemm(a, w, torch.empty(300, 512, device=DEV), bias=b, act='gelu')
    want = F.gelu(pre, approximate='tanh')
    ref = F.gelu(a.double() @ w.double().T + b.double(), approximate='tanh')
    EB.check(out, ref, EB.gemm_bound(a, w, torch.float32, bias=b, act='gelu_tanh', mode='fp32'), 'gemm fp32 tanh GELU')
    assert (out - want).abs().max().item() <= 4e-7 * max(1.0, pre.abs().max().item())        # fp32 rounding of the same pre-activation
    assert (out - erf).abs().max().item() > 1e-4                  # not the erf GELU
    # every 16-bit kernel refuses act 3 instead of computing something else; so does the split-f16 fp32 mode, which runs 16-bit GEMMs
    for dt in (torch.bfloat16, torch.float16):
        for M in (64, 4096):
            with pytest.raises(RuntimeError, match='act 3'):
                hip.gemm(torch.zeros(M, 256, dtype=dt, device=DEV), torch.zeros(512, 256, dtype=dt, device=DEV),
                         torch.empty(M, 512, device=DEV), act='gelu_tanh')
    with precision('fp32'):
        with pytest.raises(RuntimeError, match='act 3'):
            hip.gemm(a, w, torch.empty(300, 512, device=DEV), bias=b, act='gelu_tanh')


def test_token_ids_are_checked(fx, tiny_dir):
    from panst3r_amd import hip
    from panst3r_amd.model.text import load_siglip_tower
    tw = load_siglip_tower(tiny_dir)
    ids = fx['ids'][:3].to(DEV)
    bad = ids.clone()
    bad[1, 4] = tw.vocab
    with pytest.raises(ValueError, match='out of range'):
        tw.embed(bad)
    bad[1, 4] = -1
    with pytest.raises(ValueError, match='out of range'):
        tw.embed(bad)
    # the kernel's own guard: a bad id is never dereferenced, its row is zeros and the status word says PST_EINVAL
    pk = tw._pack(torch.device(DEV))
    out = torch.full((3 * 64, tw.D), 7.0, device=DEV)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    bad[1, 4] = 1 << 30
    hip.token_embed(bad.int().contiguous(), pk['tok'], pk['pos'], out, st)
    assert int(st.item()) == -1
    assert torch.count_nonzero(out[64 + 4]).item() == 0
    good = pk['tok'][ids.long()] + pk['pos'][:64][None]
    keep = torch.ones(3 * 64, dtype=torch.bool)
    keep[64 + 4] = False
    assert torch.equal(out[keep.to(DEV)], good.reshape(-1, tw.D)[keep.to(DEV)])


def _tower_768(fx, path):
    """the fixture tower with a 768-wide head (PanSt3R's class embeddings are 768-d): the e2e tests need the width, not the reference's bits"""
    g = torch.Generator().manual_seed(11)
    T.write_tower(fx, path, tokenizer=True, config=dict(fx['config'], projection_size=768), drop=('head.weight', 'head.bias'),
                  extra={'head.weight': torch.randn(768, 128, generator=g) * 0.1, 'head.bias': torch.randn(768, generator=g) * 0.1})
    return path


def test_end_to_end_set_vocab_live_mode_and_graphs(fx, tmp_path):
    import tiny
    H, W, V, K = 64, 96, 3, 2
    imgs = [i.to(DEV) for i in tiny.images(V, H, W)]
    ts = torch.tensor([[H, W]] * V)
    m = tiny.build(tiny.hip_ns(), 'v1').to(DEV)
    m.load_text_encoder(_tower_768(fx, str(tmp_path / 'tw')))
    te = m.panoptic_decoder.text_encoder
    A, B = ['chair', 'sofa', 'potted plant', 'lamp', 'door'], ['wall', 'floor', 'bed', 'window', 'tv']
    run = lambda names, **kw: m.forward_inference_multi_ar(imgs, ts, names, num_keyframes=K, amp='fp16', max_bs=1, **kw)[1]

    m.set_vocab(A)                                      # no embeddings=: the tower embeds the classes and replaces the store
    assert list(te.class_embeddings) == A
    o1 = run(A)
    rows = torch.stack([te.class_embeddings[c] for c in A]).clone()
    m.set_vocab(A, embeddings=rows)
    o2 = run(A)
    assert torch.equal(o1['pred_logits'], o2['pred_logits'])
    assert all(torch.equal(x, y) for x, y in zip(o1['pred_masks'], o2['pred_masks']))

    te.change_mode(fixed_vocab=False)                   # live mode: the classes of the call, not the store
    m.set_vocab(B)
    o3 = run(A)
    assert torch.equal(o1['pred_logits'], o3['pred_logits'])

    g1 = run(A, cache_graphs=True)
    g2 = run(B, cache_graphs=True)
    assert not torch.equal(g2['pred_logits'], g1['pred_logits'])
    g3 = run(A, cache_graphs=True)                      # second call with A: captured graphs, which must hold A's embeddings, not B's
    g4 = run(B, cache_graphs=True)
    assert torch.equal(g1['pred_logits'], o1['pred_logits']) and torch.equal(g3['pred_logits'], o1['pred_logits'])
    assert torch.equal(g4['pred_logits'], g2['pred_logits'])
    assert all(torch.equal(x, y) for x, y in zip(g3['pred_masks'], o1['pred_masks']))
