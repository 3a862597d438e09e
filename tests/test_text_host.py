"""SigLIP text tower, host side (no GPU): checkpoint layouts, key checks, local HF-cache resolution, the missing-tower error, state-dict isolation,
lazy transformers import, ABI 20."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import abi_header
import text_tiny as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def fx():
    return T.fixture()


@pytest.fixture
def empty_hub(tmp_path, monkeypatch):
    """a Hugging Face cache with nothing in it, offline"""
    hub = tmp_path / 'hub'
    hub.mkdir()
    monkeypatch.setenv('HF_HUB_CACHE', str(hub))
    monkeypatch.setenv('HF_HOME', str(tmp_path / 'hf_home'))
    monkeypatch.setenv('HF_HUB_OFFLINE', '1')
    return hub


@pytest.mark.parametrize('layout,fmt', [('bare', 'safetensors'), ('prefixed', 'safetensors'), ('full', 'safetensors'), ('bare', 'sharded'),
                                        ('full', 'bin')])
def test_loader_layouts(tmp_path, fx, layout, fmt):
    from panst3r_amd.model.text import load_siglip_tower
    tw = load_siglip_tower(T.write_tower(fx, str(tmp_path / 'm'), layout=layout, fmt=fmt), tokenizer=False)
    assert set(tw.w) == set(fx['weights'])
    for k, v in fx['weights'].items():
        assert torch.equal(tw.w[k], v), k
    assert (tw.D, tw.H, tw.hd, tw.num_layers, tw.I, tw.P, tw.npos) == (128, 2, 64, 2, 256, 128, 64)
    assert tw.eps == 1e-6


def test_loader_rejects_missing_and_extra_keys(tmp_path, fx):
    from panst3r_amd.model.text import load_siglip_tower
    with pytest.raises(RuntimeError, match='missing.*encoder.layers.1.mlp.fc2.bias'):
        load_siglip_tower(T.write_tower(fx, str(tmp_path / 'a'), drop=('encoder.layers.1.mlp.fc2.bias',)), tokenizer=False)
    with pytest.raises(RuntimeError, match='unexpected.*encoder.layers.2.layer_norm1.weight'):
        load_siglip_tower(T.write_tower(fx, str(tmp_path / 'b'), extra={'encoder.layers.2.layer_norm1.weight': torch.ones(128)}), tokenizer=False)
    # in a full SiglipModel checkpoint, only vision_model.* / logit_scale / logit_bias are ignorable: a stray text key still raises
    with pytest.raises(RuntimeError, match='unexpected.*head.extra'):
        load_siglip_tower(T.write_tower(fx, str(tmp_path / 'c'), layout='full', extra={'head.extra': torch.ones(2)}), tokenizer=False)


def test_loader_rejects_unsupported_configs(tmp_path, fx):
    from panst3r_amd.model.text import load_siglip_tower
    with pytest.raises(ValueError, match='gelu_pytorch_tanh'):
        load_siglip_tower(T.write_tower(fx, str(tmp_path / 'a'), config=dict(fx['config'], hidden_act='gelu')), tokenizer=False)
    with pytest.raises(ValueError, match='head dim'):
        load_siglip_tower(T.write_tower(fx, str(tmp_path / 'b'), config=dict(fx['config'], num_attention_heads=4)), tokenizer=False)


def test_missing_tower_still_raises(empty_hub):
    from panst3r_amd.model.panoptic import TextEncoder
    te = TextEncoder('siglip')
    with pytest.raises(NotImplementedError, match='SigLIP'):
        te.set_vocab(['chair', 'sofa'])
    with pytest.raises(NotImplementedError, match='SigLIP'):
        te.change_mode(fixed_vocab=False)
    assert te.fixed_vocab
    te.set_vocab(['chair'], embeddings=torch.ones(1, 768))       # the embeddings= path and the validate-only path are as before
    te.set_vocab(['chair'])


def test_clip_names_what_is_missing(empty_hub):
    from panst3r_amd.model.panoptic import TextEncoder
    with pytest.raises(NotImplementedError, match='causal mask.*EOS.*quick-GELU.*512'):
        TextEncoder('clip').set_vocab(['chair'])


def test_hf_cache_resolution(tmp_path, fx, empty_hub):
    pytest.importorskip('transformers')
    from panst3r_amd.model import text
    from panst3r_amd.model.panoptic import TextEncoder
    assert text.hf_cache_snapshot('google/siglip-base-patch16-224') is None
    snap = T.fake_hub(str(empty_hub), 'google/siglip-base-patch16-224', fx)
    assert text.hf_cache_snapshot('google/siglip-base-patch16-224') == snap
    assert text.hf_cache_snapshot('google/siglip2-base-patch16-224') is None
    te = TextEncoder('siglip')
    te.change_mode(fixed_vocab=False)              # resolves from the cache: the reference's Gradio call (gradio_panst3r.py:40)
    assert not te.fixed_vocab and te.tower().source == snap
    assert te.tower().tokenizer is not None
    with pytest.raises(NotImplementedError, match='SigLIP'):
        TextEncoder('siglip2').change_mode(fixed_vocab=False)     # a different hub id: not in the cache
    # HF_HOME/hub is the fallback when HF_HUB_CACHE is unset
    os.environ.pop('HF_HUB_CACHE')
    home_hub = tmp_path / 'hf_home' / 'hub'
    T.fake_hub(str(home_hub), 'google/siglip2-base-patch16-224', fx)
    assert text.hf_cache_snapshot('google/siglip2-base-patch16-224').startswith(str(home_hub))


def test_tower_not_in_state_dict(tmp_path, fx, empty_hub):
    pytest.importorskip('transformers')
    import tiny
    m = tiny.build(tiny.hip_ns(), 'v1')
    before = {k: v.clone() for k, v in m.state_dict().items()}
    tw = m.load_text_encoder(T.write_tower(fx, str(tmp_path / 'm'), tokenizer=True))
    assert tw is m.panoptic_decoder.text_encoder.tower()
    after = m.state_dict()
    assert set(after) == set(before)
    assert not any('text_encoder' in k for k in after)
    assert all(torch.equal(after[k], before[k]) for k in before)
    assert not any(p is t for p in m.parameters() for t in tw.w.values())
    from panst3r_amd.panst3r import check_checkpoint_keys
    check_checkpoint_keys(m.load_state_dict(dict(before, **{'panoptic_decoder.text_encoder.model.head.weight': torch.zeros(1)}), strict=False))


def test_embed_refuses_cpu_tensors(tmp_path, fx):
    from panst3r_amd.model.text import load_siglip_tower
    tw = load_siglip_tower(T.write_tower(fx, str(tmp_path / 'm')), tokenizer=False)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        tw.embed(fx['ids'][:2])


def test_import_does_not_pull_in_transformers():
    code = ('import sys; import panst3r_amd, panst3r_amd.panst3r, panst3r_amd.ops, panst3r_amd.model.text; '
            'bad = sorted(m for m in sys.modules if m.split(".")[0] == "transformers"); assert not bad, bad')
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_abi_20_exports_the_text_tower():
    from panst3r_amd.build import build
    from panst3r_amd import hip
    import panst3r_amd.ops as O
    assert hip.ABI_VERSION == 20
    assert 'pst_token_embed' in hip.EXPORTS
    lib = ctypes.CDLL(build(verbose=False))
    lib.pst_abi_version.restype = ctypes.c_int
    assert lib.pst_abi_version() == 20 and hasattr(lib, 'pst_token_embed')
    assert hip.ACT['gelu_tanh'] == 3
    assert 'token_embed' in O.registered_ops() and hasattr(torch.ops.panst3r_hip, 'token_embed')
    assert abi_header.defines()['PST_ABI_VERSION'] == 20
