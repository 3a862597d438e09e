"""SigLIP text tower on the HIP kernels: the live-vocabulary half of the reference's TextEncoder (src/panst3r/model/text_encoder.py:44-103).

The tower (transformers SiglipTextModel / Siglip2TextModel, the same graph with a different vocabulary and tokenizer):
    x      = tok_emb[ids] + pos_emb[0 .. L)                                      token gather (csrc/text.hip)
    N x    x += out_proj( MHA( LN1(x) ) )      pre-LN, bias everywhere, head dim 64, no causal mask, the tokenizer's key-padding mask
           x += fc2( gelu_tanh( fc1( LN2(x) ) ) )                                LayerNorm eps 1e-6, tanh-approximate GELU (gemm act 3)
    pooled = head( final_LN( x[:, L - 1] ) )                                     the LAST position, padding or not
Everything runs on the exact-fp32 kernels (gemm_f32.hip / attn_f32.hip, precision 'fp32_exact') whatever the caller's precision: the reference computes
the tower in fp32 outside its autocast (panst3r.py:236-245), it runs once per vocabulary, and the split-f16 mode has the f16 range limit of its hi part.
Only the pooled rows go through the last layer's query / output projection / MLP, the final LayerNorm and the head (the keys and values of the last
layer still cover every position): the same arithmetic per pooled row as the full stack.

Weights come from a LOCAL directory (config.json + model.safetensors / a sharded model.safetensors.index.json / pytorch_model.bin) or from the local
Hugging Face cache under the reference's hub id; nothing here touches the network.  `transformers` is imported for the tokenizer only, lazily.
"""
import json
import os

import torch

from .. import hip
from .common import precision

# reference text_encoder.py:7-30 (the released configs use 'siglip': configs/base.yaml:25, base_v2.yaml:24)
MODEL_CONFIGS = {
    'siglip': dict(hf_model='google/siglip-base-patch16-224', template='This is a photo of {}.', tokenizer_args=dict(padding='max_length')),
    'siglip2': dict(hf_model='google/siglip2-base-patch16-224', template='this is a photo of {}', tokenizer_args=dict(padding='max_length', max_length=64)),
}
BATCH = 32                                # reference embed_classes(bs=32)
CLIP_MISSING = ("text_encoder='clip' has no text tower in this build: the CLIP text model needs a causal mask, EOS-token pooling, quick-GELU and "
                "512-d outputs, none of which the SigLIP tower here implements (no released PanSt3R config uses CLIP)")

# SiglipTextConfig defaults (what a full SiglipModel config.json leaves out of its text_config)
_DEFAULTS = dict(num_attention_heads=12, hidden_act='gelu_pytorch_tanh', layer_norm_eps=1e-6)
_IGNORED_FULL = ('vision_model.', 'logit_scale', 'logit_bias')
_LAYER_KEYS = ('layer_norm1.weight', 'layer_norm1.bias', 'self_attn.q_proj.weight', 'self_attn.q_proj.bias', 'self_attn.k_proj.weight',
               'self_attn.k_proj.bias', 'self_attn.v_proj.weight', 'self_attn.v_proj.bias', 'self_attn.out_proj.weight', 'self_attn.out_proj.bias',
               'layer_norm2.weight', 'layer_norm2.bias', 'mlp.fc1.weight', 'mlp.fc1.bias', 'mlp.fc2.weight', 'mlp.fc2.bias')
_TOP_KEYS = ('embeddings.token_embedding.weight', 'embeddings.position_embedding.weight', 'final_layer_norm.weight', 'final_layer_norm.bias',
             'head.weight', 'head.bias')


def expected_keys(num_layers):
    return set(_TOP_KEYS) | {'encoder.layers.%d.%s' % (i, k) for i in range(num_layers) for k in _LAYER_KEYS}


class SiglipTextTower:
    """Weights of a SigLIP text tower (fp32, host) + `embed`, which launches HIP ops only.  Not an nn.Module: the tower is not part of a PanSt3R
    state dict (its weights live in their own checkpoint, next to the tokenizer)."""

    def __init__(self, config, weights, tokenizer=None, source=None):
        cfg = dict(_DEFAULTS, **{k: v for k, v in config.items() if v is not None})
        if cfg['hidden_act'] != 'gelu_pytorch_tanh':
            raise ValueError('SigLIP text tower: hidden_act %r is not supported (the tower runs gelu_pytorch_tanh, the tanh-approximate GELU)' % cfg['hidden_act'])
        self.num_layers = int(cfg.get('num_hidden_layers', sum(1 for k in weights if k.endswith('.layer_norm1.weight'))))
        want = expected_keys(self.num_layers)
        missing, unexpected = sorted(want - set(weights)), sorted(set(weights) - want)
        if missing or unexpected:
            raise RuntimeError('SigLIP text tower checkpoint does not match a %d-layer SiglipTextModel.\n  missing (%d): %s\n  unexpected (%d): %s'
                               % (self.num_layers, len(missing), ', '.join(missing[:8]), len(unexpected), ', '.join(unexpected[:8])))
        self.w = {k: v.detach().float().contiguous() for k, v in weights.items()}
        self.vocab, self.D = self.w['embeddings.token_embedding.weight'].shape
        self.npos = self.w['embeddings.position_embedding.weight'].shape[0]
        self.I = self.w['encoder.layers.0.mlp.fc1.weight'].shape[0]
        self.P = self.w['head.weight'].shape[0]
        self.H = int(cfg['num_attention_heads'])
        self.eps = float(cfg['layer_norm_eps'])
        if self.D % self.H or self.D // self.H not in (64, 96):
            raise ValueError('SigLIP text tower: head dim %d / %d heads: the fp32 attention kernel takes head dim 64 or 96' % (self.D, self.H))
        if self.D % 16 or self.I % 16 or self.P % 4:
            raise ValueError('SigLIP text tower: the fp32 GEMM needs hidden / intermediate sizes that are multiples of 16 (got %d, %d) and a head '
                             'width multiple of 4 (got %d)' % (self.D, self.I, self.P))
        self.hd = self.D // self.H
        self.tokenizer, self.source = tokenizer, source
        self._dev = {}

    # ---------------------------------------------------------------------------------------------------- device copies
    def _pack(self, device):
        pk = self._dev.get(str(device))
        if pk is not None:
            return pk
        w = self.w
        g = lambda k: w[k].to(device)
        pos = w['embeddings.position_embedding.weight']
        npad = -(-self.npos // 8) * 8              # sequences run padded to a multiple of 8 positions (attention strides); pad rows are masked keys
        pos_pad = torch.zeros(npad, self.D)
        pos_pad[:self.npos] = pos
        pk = dict(tok=g('embeddings.token_embedding.weight'), pos=pos_pad.to(device), layers=[],
                  lnf=(g('final_layer_norm.weight'), g('final_layer_norm.bias')), head=(g('head.weight'), g('head.bias')))
        for i in range(self.num_layers):
            p = 'encoder.layers.%d.' % i
            pk['layers'].append(dict(
                ln1=(g(p + 'layer_norm1.weight'), g(p + 'layer_norm1.bias')), ln2=(g(p + 'layer_norm2.weight'), g(p + 'layer_norm2.bias')),
                wqk=torch.cat([w[p + 'self_attn.q_proj.weight'], w[p + 'self_attn.k_proj.weight']]).to(device).contiguous(),
                bqk=torch.cat([w[p + 'self_attn.q_proj.bias'], w[p + 'self_attn.k_proj.bias']]).to(device).contiguous(),
                wv=g(p + 'self_attn.v_proj.weight'), bv=g(p + 'self_attn.v_proj.bias'),
                wo=g(p + 'self_attn.out_proj.weight'), bo=g(p + 'self_attn.out_proj.bias'),
                w1=g(p + 'mlp.fc1.weight'), b1=g(p + 'mlp.fc1.bias'), w2=g(p + 'mlp.fc2.weight'), b2=g(p + 'mlp.fc2.bias')))
        self._dev[str(device)] = pk
        return pk

    # ---------------------------------------------------------------------------------------------------- forward
    @torch.no_grad()
    def embed(self, input_ids, attention_mask=None):
        """pooler_output of SiglipTextModel(input_ids, attention_mask): [B, P] fp32 on the ids' device, before any normalisation.
        input_ids [B, L] (any integer dtype) on the GPU; attention_mask [B, L] (1 = token, 0 = padding) or None = every position attends."""
        if not input_ids.is_cuda:
            raise RuntimeError('panst3r_amd HIP op got a %s tensor: the HIP path runs on the GPU only (no CPU fallback)' % input_ids.device)
        if input_ids.dim() != 2:
            raise ValueError('input_ids must be [B, L], got %s' % (tuple(input_ids.shape),))
        B, L = input_ids.shape
        if L > self.npos:
            raise ValueError('sequence length %d exceeds the %d position embeddings of the text tower' % (L, self.npos))
        if B == 0:
            return torch.empty(0, self.P, dtype=torch.float32, device=input_ids.device)
        bad = (input_ids < 0) | (input_ids >= self.vocab)
        if bool(bad.any()):
            raise ValueError('token id out of range [0, %d): %d' % (self.vocab, int(input_ids[bad][0])))
        with precision('fp32_exact'):             # restores the caller's context on exit
            return self._run(input_ids, attention_mask)

    def _run(self, input_ids, attention_mask):
        dev = input_ids.device
        pk = self._pack(dev)
        B, L = input_ids.shape
        Lp = -(-L // 8) * 8                        # V^T batch stride and Q / K row blocks: multiples of 8 elements
        D, H, hd, R = self.D, self.H, self.hd, B * Lp
        ids = torch.zeros(B, Lp, dtype=torch.int32, device=dev)
        ids[:, :L] = input_ids
        mask = None
        if attention_mask is not None or Lp != L:  # uint8 [B, Lp], 1 = blocked key (attn_f32.hip), shared by all heads and query rows (m_rs = 0)
            mask = torch.ones(B, Lp, dtype=torch.uint8, device=dev)
            mask[:, :L] = 0 if attention_mask is None else (attention_mask.to(dev) == 0).to(torch.uint8)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        x = torch.empty(R, D, dtype=torch.float32, device=dev)
        hip.token_embed(ids, pk['tok'], pk['pos'], x, status)
        h = torch.empty_like(x)
        vt = torch.empty(D, R, dtype=torch.float32, device=dev)
        attn = dict(B=B, H=H, Nk=Lp, hd=hd, v_strides=(Lp, hd * R, R), mask=mask, mask_strides=(Lp, 0))
        last = len(pk['layers']) - 1
        for i, ly in enumerate(pk['layers']):
            hip.layernorm(x, ly['ln1'][0], ly['ln1'][1], h, self.eps)
            hip.gemm(h, ly['wv'], vt, bias=ly['bv'], trans_out=True)
            if i < last:
                qk = torch.empty(R, 2 * D, dtype=torch.float32, device=dev)
                hip.gemm(h, ly['wqk'], qk, bias=ly['bqk'])
                o = torch.empty(R, D, dtype=torch.float32, device=dev)
                hip.attention(qk, qk[:, D:], vt, o, Nq=Lp, q_strides=(Lp * 2 * D, hd, 2 * D), k_strides=(Lp * 2 * D, hd, 2 * D),
                              o_strides=(Lp * D, hd, D), **attn)
                hip.gemm(o, ly['wo'], x, bias=ly['bo'], res=x)
                hip.layernorm(x, ly['ln2'][0], ly['ln2'][1], h, self.eps)
                f = torch.empty(R, self.I, dtype=torch.float32, device=dev)
                hip.gemm(h, ly['w1'], f, bias=ly['b1'], act='gelu_tanh')
                hip.gemm(f, ly['w2'], x, bias=ly['b2'], res=x)
                continue
            # last layer: keys / values of every position, everything else for the pooled position L - 1 only
            k = torch.empty(R, D, dtype=torch.float32, device=dev)
            hip.gemm(h, ly['wqk'][D:], k, bias=ly['bqk'][D:])
            q = torch.empty(B, D, dtype=torch.float32, device=dev)
            hip.gemm(h.view(B, Lp, D)[:, L - 1], ly['wqk'][:D], q, bias=ly['bqk'][:D])
            o = torch.empty(B, D, dtype=torch.float32, device=dev)
            hip.attention(q, k, vt, o, Nq=1, q_strides=(D, hd, D), k_strides=(Lp * D, hd, D), o_strides=(D, hd, D), **attn)
            xp = torch.empty(B, D, dtype=torch.float32, device=dev)
            hip.gemm(o, ly['wo'], xp, bias=ly['bo'], res=x.view(B, Lp, D)[:, L - 1])
            hp = torch.empty_like(xp)
            hip.layernorm(xp, ly['ln2'][0], ly['ln2'][1], hp, self.eps)
            f = torch.empty(B, self.I, dtype=torch.float32, device=dev)
            hip.gemm(hp, ly['w1'], f, bias=ly['b1'], act='gelu_tanh')
            hip.gemm(f, ly['w2'], xp, bias=ly['b2'], res=xp)
        y = torch.empty(B, D, dtype=torch.float32, device=dev)
        hip.layernorm(xp, pk['lnf'][0], pk['lnf'][1], y, self.eps)
        out = torch.empty(B, self.P, dtype=torch.float32, device=dev)
        hip.gemm(y, pk['head'][0], out, bias=pk['head'][1])
        if int(status.item()) != 0:               # the kernel's own bounds guard (the host check above makes this unreachable)
            raise RuntimeError('pst_token_embed: a token id outside the vocabulary reached the kernel')
        return out

    # ---------------------------------------------------------------------------------------------------- text -> embeddings
    def embed_texts(self, texts, tokenizer_args, device, bs=BATCH):
        """reference embed_classes: tokenize in batches of `bs`, the tokenizer's whole output (input_ids and, when it returns one, attention_mask)
        into the tower; [len(texts), P] fp32 pooled rows on `device`."""
        if self.tokenizer is None:
            raise RuntimeError('SigLIP text tower from %s has no tokenizer (tokenizer files next to the weights)' % (self.source,))
        batches = []
        for i in range(0, len(texts), bs):
            enc = self.tokenizer(list(texts[i:i + bs]), return_tensors='pt', **tokenizer_args)
            batches.append((enc['input_ids'], enc['attention_mask'] if 'attention_mask' in enc else None))
        if not batches:
            return torch.empty(0, self.P, dtype=torch.float32, device=device)
        if len({b[0].shape[1] for b in batches}) == 1 and len({b[1] is None for b in batches}) == 1:
            # padding='max_length': every batch has the same length, so they run as ONE tower pass (rows are independent: same bits per row as
            # batch by batch, fewer and fuller launches)
            ids = torch.cat([b[0] for b in batches])
            am = None if batches[0][1] is None else torch.cat([b[1] for b in batches])
            batches = [(ids, am)]
        return torch.cat([self.embed(ids.to(device), None if am is None else am.to(device)) for ids, am in batches])


# -------------------------------------------------------------------------------------------------------- loading
def _read_state(path):
    st = os.path.join(path, 'model.safetensors')
    idx = os.path.join(path, 'model.safetensors.index.json')
    binf = os.path.join(path, 'pytorch_model.bin')
    if os.path.exists(st) or os.path.exists(idx):
        from safetensors.torch import load_file
        if os.path.exists(st):
            return load_file(st)
        shards = sorted(set(json.load(open(idx))['weight_map'].values()))
        out = {}
        for s in shards:
            out.update(load_file(os.path.join(path, s)))
        return out
    if os.path.exists(binf):
        return torch.load(binf, map_location='cpu', weights_only=True)
    raise FileNotFoundError('no model.safetensors, model.safetensors.index.json or pytorch_model.bin in %s' % path)


def tower_state(config, state):
    """(text config, tower weights under the bare SiglipTextModel keys) from a checkpoint in any of the three layouts: a bare SiglipTextModel, the same
    keys under `text_model.`, or a full SiglipModel / Siglip2Model (text_config + text_model.*; vision_model.*, logit_scale, logit_bias ignored)."""
    if 'text_config' in config:
        tcfg = dict(config['text_config'] or {})
        state = {k: v for k, v in state.items() if not k.startswith(_IGNORED_FULL)}
    else:
        tcfg = dict(config)
    if any(k.startswith('text_model.') for k in state):
        state = {(k[len('text_model.'):] if k.startswith('text_model.') else k): v for k, v in state.items()}
    return tcfg, state


def load_tokenizer(path):
    from transformers import AutoTokenizer          # lazily: `import panst3r_amd` never pulls in transformers
    return AutoTokenizer.from_pretrained(path, local_files_only=True)


def load_siglip_tower(path, tokenizer=True):
    """SiglipTextTower from a local directory (config.json + weights, tokenizer files optional with tokenizer=True)."""
    path = os.fspath(path)
    cfg_file = os.path.join(path, 'config.json')
    if not os.path.isfile(cfg_file):
        raise FileNotFoundError('no config.json in %s' % path)
    tcfg, state = tower_state(json.load(open(cfg_file)), _read_state(path))
    tok = None
    if tokenizer:
        try:
            tok = load_tokenizer(path)
        except Exception as e:                      # missing files, a tokenizer class this install lacks, ...
            raise RuntimeError('SigLIP text tower at %s: no usable tokenizer (%s)' % (path, e)) from e
    return SiglipTextTower(tcfg, state, tok, source=path)


def hf_cache_snapshot(repo_id):
    """local snapshot directory of `repo_id` in the Hugging Face hub cache (HF_HUB_CACHE, else HF_HOME/hub, else ~/.cache/huggingface/hub), or None.
    Reads the cache layout only (models--org--name/refs/main -> snapshots/<commit>): never a network call."""
    cache = os.environ.get('HF_HUB_CACHE') or os.environ.get('HUGGINGFACE_HUB_CACHE')
    if not cache:
        home = os.environ.get('HF_HOME') or os.path.join(os.environ.get('XDG_CACHE_HOME') or os.path.join(os.path.expanduser('~'), '.cache'), 'huggingface')
        cache = os.path.join(home, 'hub')
    repo = os.path.join(cache, 'models--' + repo_id.replace('/', '--'))
    snaps = os.path.join(repo, 'snapshots')
    if not os.path.isdir(snaps):
        return None
    ref = os.path.join(repo, 'refs', 'main')
    cands = []
    if os.path.isfile(ref):
        cands.append(os.path.join(snaps, open(ref).read().strip()))
    cands += sorted((os.path.join(snaps, d) for d in os.listdir(snaps)), key=os.path.getmtime, reverse=True)
    for c in cands:
        if os.path.isfile(os.path.join(c, 'config.json')) and any(
                os.path.exists(os.path.join(c, f)) for f in ('model.safetensors', 'model.safetensors.index.json', 'pytorch_model.bin')):
            return c
    return None


def resolve_tower(model_name, path=None):
    """The text tower of `model_name`: from `path` if given, else the reference's hub id in the local HF cache; None when neither resolves."""
    if model_name == 'clip':
        raise NotImplementedError(CLIP_MISSING)
    if path is not None:
        return load_siglip_tower(path)
    snap = hf_cache_snapshot(MODEL_CONFIGS[model_name]['hf_model'])
    return None if snap is None else load_siglip_tower(snap)
