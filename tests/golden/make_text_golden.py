#!/usr/bin/env python
"""Generate tests/golden/text_siglip_tiny.npz with the REFERENCE's own TextEncoder (build container only, like make_golden.py).

Run:  python tests/golden/make_text_golden.py <reference checkout>     (a checkout of naver/panst3r, or PANST3R_REFERENCE; needs transformers and
      sentencepiece; build container only, never on the GPU box)

The reference's src/panst3r/model/text_encoder.py needs only torch and transformers: it is imported through a bare package stub.  Its `get_model`
(which would download google/siglip-base-patch16-224) is replaced by a seeded SMALL transformers SiglipTextModel (hidden 128, 2 heads x 64,
2 layers, intermediate 256, 64 positions) and a SiglipTokenizer on a sentencepiece model trained here.  The reference's `set_vocab` and
`forward` (fixed vocabulary, then live mode) then run unchanged in fp32 on the CPU.

The weights are drawn, then rounded to int8 multiples of a power of two per tensor (q * 2^e is exact in fp32) BEFORE the reference runs, so that
they can be stored as int8 (the file stays small) and rebuilt bit-exactly (tests/text_tiny.py).
Written (data only): the tower weights under their SiglipTextModel keys (q/<key> int8, e/<key> exponent), its config (json), the sentencepiece model bytes, the class
names (one longer than the template, one that tokenizes to <unk>), the expected store (pooled rows, set_vocab) and the forward output
(unit-norm rows), in both modes.
"""
import importlib
import io
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'text_siglip_tiny.npz')

CLASSES = ['chair', 'sofa', 'table', 'potted plant', 'person',
           'large wooden dining table with four matching chairs next to the window',       # longer than the template
           'æøå',                                                               # characters the spm model never saw: <unk>
           'wall', 'floor', 'ceiling', 'door', 'window', 'lamp', 'bed', 'tv']
CONFIG = dict(vocab_size=None, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, max_position_embeddings=64,
              hidden_act='gelu_pytorch_tanh', layer_norm_eps=1e-6, projection_size=128)


def import_reference(checkout):
    REF = os.path.join(checkout, 'src', 'panst3r')

    def pkg(name, path=None):
        m = types.ModuleType(name)
        m.__path__ = [path] if path else []
        sys.modules[name] = m
        return m
    pkg('panst3r', REF)
    pkg('panst3r.model', REF + '/model')
    return importlib.import_module('panst3r.model.text_encoder')


def train_spm():
    import sentencepiece as spm
    words = ['chair', 'sofa', 'table', 'potted', 'plant', 'person', 'large', 'wooden', 'dining', 'with', 'four', 'matching', 'chairs', 'next',
             'to', 'the', 'window', 'wall', 'floor', 'ceiling', 'door', 'lamp', 'bed', 'tv', 'cat', 'dog', 'car', 'tree', 'road', 'sky']
    rng = np.random.default_rng(5)
    corpus = ['This is a photo of %s.' % ' '.join(rng.choice(words, size=int(rng.integers(1, 4)))) for _ in range(400)]
    buf = io.BytesIO()
    # pad must differ from eos for the trainer; the SigLIP tokenizer pads with </s> (= eos) as the released one does
    spm.SentencePieceTrainer.train(sentence_iterator=iter(corpus), model_writer=buf, vocab_size=160, model_type='unigram', pad_id=0, eos_id=1,
                                   unk_id=2, bos_id=-1, hard_vocab_limit=False, character_coverage=1.0)
    return buf.getvalue()


def tokenizer_from(spm_bytes, tmp):
    from transformers import SiglipTokenizer
    f = os.path.join(tmp, 'spiece.model')
    open(f, 'wb').write(spm_bytes)
    return SiglipTokenizer(vocab_file=f, model_max_length=64)


def quantize_(t):
    """round t in place to q * 2^e with q in int8 (e per tensor); returns (q int8, e)"""
    e = int(np.ceil(np.log2(max(float(t.abs().max()), 1e-30) / 127.0)))
    q = torch.round(t / 2.0 ** e).clamp_(-127, 127)
    t.copy_(q * 2.0 ** e)
    return q.to(torch.int8).numpy(), e


def main():
    from transformers import SiglipTextConfig, SiglipTextModel
    checkout = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('PANST3R_REFERENCE')
    if not checkout:
        sys.exit('usage: make_text_golden.py <checkout of naver/panst3r>   (or set PANST3R_REFERENCE)')
    ref = import_reference(checkout)
    spm_bytes = train_spm()
    with tempfile.TemporaryDirectory() as tmp:
        tok = tokenizer_from(spm_bytes, tmp)
        cfg = dict(CONFIG, vocab_size=len(tok))
        torch.manual_seed(1234)
        model = SiglipTextModel(SiglipTextConfig(**cfg)).eval()
        with torch.no_grad():                 # larger-than-init weights so that every term of the tower moves the pooled row
            for k, v in model.state_dict().items():
                if v.dim() == 2 or k.endswith('bias'):
                    v.normal_(0.0, 0.08 if v.dim() == 2 else 0.05)
            qe = {k: quantize_(v) for k, v in model.state_dict().items()}
        ref.TextEncoder.get_model = lambda self: (model, tok)
        te = ref.TextEncoder('siglip', fixed_vocab=True)
        te.set_vocab(CLASSES)
        store = torch.stack([te.class_embeddings[c] for c in CLASSES])
        fwd = te(CLASSES)
        te.change_mode(fixed_vocab=False)
        fwd_live = te(CLASSES)
        ids = tok([ref.MODEL_CONFIGS['siglip']['template'].format(c) for c in CLASSES], return_tensors='pt', padding='max_length')['input_ids']
    assert int((ids == tok.unk_token_id).sum()) > 0, 'the <unk> class did not tokenize to <unk>'
    out = {}
    for k, (q, e) in qe.items():
        out['q/' + k], out['e/' + k] = q, np.array(e, dtype=np.int32)
    out.update(config=np.array(json.dumps(cfg)), spm=np.frombuffer(spm_bytes, dtype=np.uint8), classes=np.array(CLASSES),
               ids=ids.numpy().astype(np.int32), store=store.numpy(), forward=fwd.numpy(), forward_live=fwd_live.numpy())
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes; tokens per class', (ids != tok.pad_token_id).sum(1).tolist())


if __name__ == '__main__':
    main()
