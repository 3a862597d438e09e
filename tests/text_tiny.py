"""The tiny SigLIP text tower of tests/golden/text_siglip_tiny.npz (written by tests/golden/make_text_golden.py from the reference's TextEncoder) as
local checkpoint directories in the layouts the loader accepts."""
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'text_siglip_tiny.npz')


def fixture():
    z = np.load(GOLDEN)
    # int8 multiples of a power of two per tensor (make_text_golden.py rounds the weights so before the reference runs): rebuilt exactly in fp32
    weights = {k[2:]: torch.from_numpy(z[k].astype(np.float32)) * 2.0 ** int(z['e/' + k[2:]]) for k in z.files if k.startswith('q/')}
    return dict(weights=weights, config=json.loads(str(z['config'])),
                spm=z['spm'].tobytes(), classes=[str(c) for c in z['classes']], ids=torch.from_numpy(z['ids']),
                store=torch.from_numpy(z['store']), forward=torch.from_numpy(z['forward']), forward_live=torch.from_numpy(z['forward_live']))


def write_tokenizer(fx, path):
    """SiglipTokenizer on the fixture's sentencepiece model, saved next to the weights (needs transformers + sentencepiece; no network)"""
    from transformers import SiglipTokenizer
    os.makedirs(path, exist_ok=True)
    spm = os.path.join(path, 'spiece.model')
    with open(spm, 'wb') as f:
        f.write(fx['spm'])
    SiglipTokenizer(vocab_file=spm, model_max_length=64).save_pretrained(path)


def write_tower(fx, path, layout='bare', fmt='safetensors', tokenizer=False, config=None, drop=(), extra=None):
    """layout: 'bare' (SiglipTextModel keys), 'prefixed' (the same under text_model.), 'full' (a SiglipModel checkpoint: text_config, text_model.*,
    vision_model.*, logit_scale, logit_bias).  fmt: 'safetensors', 'sharded' (model.safetensors.index.json + two shards) or 'bin'."""
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    cfg = dict(fx['config'] if config is None else config)
    sd = {k: v.clone() for k, v in fx['weights'].items() if k not in drop}
    if extra:
        sd.update(extra)
    if layout in ('prefixed', 'full'):
        sd = {'text_model.' + k: v for k, v in sd.items()}
    if layout == 'full':
        sd.update({'vision_model.embeddings.patch_embedding.weight': torch.zeros(8, 3, 4, 4), 'vision_model.post_layernorm.weight': torch.ones(8),
                   'logit_scale': torch.zeros(1), 'logit_bias': torch.zeros(1)})
        cfg = dict(model_type='siglip', text_config=cfg, vision_config=dict(hidden_size=8))
    with open(os.path.join(path, 'config.json'), 'w') as f:
        json.dump(cfg, f)
    if fmt == 'safetensors':
        save_file(sd, os.path.join(path, 'model.safetensors'))
    elif fmt == 'sharded':
        keys = sorted(sd)
        parts = {'model-00001-of-00002.safetensors': keys[:len(keys) // 2], 'model-00002-of-00002.safetensors': keys[len(keys) // 2:]}
        for name, ks in parts.items():
            save_file({k: sd[k] for k in ks}, os.path.join(path, name))
        with open(os.path.join(path, 'model.safetensors.index.json'), 'w') as f:
            json.dump(dict(metadata={}, weight_map={k: n for n, ks in parts.items() for k in ks}), f)
    else:
        torch.save(sd, os.path.join(path, 'pytorch_model.bin'))
    if tokenizer:
        write_tokenizer(fx, path)
    return path


def fake_hub(root, repo_id, fx, commit='0123456789abcdef'):
    """the local Hugging Face cache layout of `repo_id` (models--org--name/refs/main + snapshots/<commit>) holding the fixture tower"""
    repo = os.path.join(root, 'models--' + repo_id.replace('/', '--'))
    os.makedirs(os.path.join(repo, 'refs'), exist_ok=True)
    with open(os.path.join(repo, 'refs', 'main'), 'w') as f:
        f.write(commit)
    return write_tower(fx, os.path.join(repo, 'snapshots', commit), layout='full', tokenizer=True)
