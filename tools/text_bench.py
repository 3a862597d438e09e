#!/usr/bin/env python
"""ms per set_vocab through the HIP SigLIP text tower (GPU box), with transformers' SiglipTextModel in fp32 eager on the same GPU as the yardstick.
    python tools/text_bench.py [--classes 133 200] [--reps 10] [--out FILE]

Full-size SigLIP-base text tower (vocab 32000, 768, 12 layers x 12 heads, 3072, 64 positions) with seeded random weights; the tokenizer is the small
sentencepiece model of tests/golden/text_siglip_tiny.npz (its ids are valid in any larger vocabulary; the sequences are padded to 64 positions either way,
which is what the tower's cost depends on).  HIP: TextEncoder.set_vocab (template, tokenizer, tower, store) from a fresh store each repetition.
Yardstick: the reference's embed_classes loop (batches of 32, model(**inputs).pooler_output) on the same token ids."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402

from panst3r_amd.model.panoptic import TextEncoder  # noqa: E402
from panst3r_amd.model.text import SiglipTextTower, MODEL_CONFIGS, expected_keys  # noqa: E402
import text_tiny  # noqa: E402

CFG = dict(vocab_size=32000, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12, max_position_embeddings=64,
           hidden_act='gelu_pytorch_tanh', layer_norm_eps=1e-6, projection_size=768)


def weights(seed=0):
    g = torch.Generator().manual_seed(seed)
    D, I, V, P = CFG['hidden_size'], CFG['intermediate_size'], CFG['vocab_size'], CFG['max_position_embeddings']
    shape = {'embeddings.token_embedding.weight': (V, D), 'embeddings.position_embedding.weight': (P, D), 'head.weight': (D, D)}
    out = {}
    for k in sorted(expected_keys(CFG['num_hidden_layers'])):
        if k in shape:
            s = shape[k]
        elif k.endswith('fc1.weight'):
            s = (I, D)
        elif k.endswith('fc2.weight'):
            s = (D, I)
        elif k.endswith('fc1.bias'):
            s = (I,)
        elif k.endswith('.weight') and 'norm' not in k:
            s = (D, D)
        else:
            s = (D,)
        out[k] = (1.0 + 0.05 * torch.randn(s, generator=g)) if 'norm' in k and k.endswith('weight') else 0.02 * torch.randn(s, generator=g)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--classes', type=int, nargs='+', default=[133, 200])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    w = weights()
    fx = text_tiny.fixture()
    with tempfile.TemporaryDirectory() as tmp:
        text_tiny.write_tokenizer(fx, tmp)
        from transformers import AutoTokenizer, SiglipTextConfig, SiglipTextModel
        tok = AutoTokenizer.from_pretrained(tmp, local_files_only=True)
    tower = SiglipTextTower(CFG, w, tok, source='random')
    te = TextEncoder('siglip')
    te._tower = tower
    ref = SiglipTextModel(SiglipTextConfig(**CFG)).eval()
    ref.load_state_dict(w, strict=True)
    ref = ref.to(dev)
    words = ['chair', 'sofa', 'table', 'potted', 'plant', 'person', 'wooden', 'dining', 'wall', 'floor', 'ceiling', 'door', 'window', 'lamp', 'bed']
    rows = []
    for n in a.classes:
        names = ['%s %s %d' % (words[i % len(words)], words[(i * 7 + 3) % len(words)], i) for i in range(n)]
        cfg = MODEL_CONFIGS['siglip']

        def hip_once():
            te.class_embeddings = {}
            te.set_vocab(names, device=dev)

        def ref_once():
            texts = [cfg['template'].format(c) for c in names]
            embs = []
            with torch.no_grad():
                for i in range(0, len(texts), 32):
                    inputs = {k: v.to(dev) for k, v in tok(texts[i:i + 32], return_tensors='pt', **cfg['tokenizer_args']).items()}
                    embs.append(ref(**inputs).pooler_output)
            return torch.cat(embs)

        def timed(f):
            for _ in range(2):
                f()
            torch.cuda.synchronize()
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            ts.sort()
            return ts[len(ts) // 2], ts[0]

        h_med, h_min = timed(hip_once)
        r_med, r_min = timed(ref_once)
        got = torch.stack([te.class_embeddings[c] for c in names])
        want = ref_once()
        err = ((got.double() - want.double()).norm(dim=-1) / want.double().norm(dim=-1)).max().item()
        row = dict(classes=n, tokens_per_class=64, hip_set_vocab_ms=round(h_med, 2), hip_min_ms=round(h_min, 2),
                   transformers_fp32_eager_ms=round(r_med, 2), transformers_min_ms=round(r_min, 2), max_rel_l2_vs_transformers_gpu=err,
                   tflop=round(2.0 * n * 64 * (12 * (4 * 768 * 768 + 2 * 768 * 3072) + 12 * 2 * 64 * 768) / 1e12, 3))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)


if __name__ == '__main__':
    main()
