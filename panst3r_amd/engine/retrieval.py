"""`PanSt3RRetriever` of the reference (src/panst3r/engine/retrieval.py:12-47) on the HIP path: same name, constructor and call.  The reference
builds it on must3r's RetrievalModel + asmk + faiss-GPU (CUDA only); here the head runs on pst_gemm / pst_layernorm in fp32 mode and ASMK on
csrc/retrieval.hip - see panst3r_amd/model/retrieval.py for the restated algorithm [3P-recalled, parity unpinned]."""
import numpy as np
import torch

from ..model.retrieval import RetrievalASMK


class PanSt3RRetriever:
    def __init__(self, ckpt, backbone, device='cuda', verbose=True):
        """ckpt: the checkpoint's `retrieval` dict, a path to a torch file holding one, or an already parsed RetrievalASMK (kept packed on the
        device between calls).  `backbone` is the scene's must3r encoder (the head's `backbone.*` keys are ignored: its features come from it)."""
        assert backbone is not None
        self.backbone = backbone
        self.model = ckpt if isinstance(ckpt, RetrievalASMK) else RetrievalASMK(ckpt)
        self.device = torch.device(device)
        self.verbose = verbose
        self.imsize = self.model.imsize

    @torch.no_grad()
    def __call__(self, must3r_x, device=None):
        """must3r_x: list[V] of encoder tokens [1, T_v, D] or [T_v, D] (views may differ in T) -> V x V similarity (numpy float32, query rows)"""
        dev = torch.device(device) if device is not None else self.device
        xs = []
        for x in must3r_x:
            x = x.reshape(-1, x.shape[-1])
            xs.append(x.to(device=dev, dtype=torch.float32).contiguous())
        if xs[0].shape[-1] != self.model.d_in:
            raise ValueError('retriever head expects %d-dim encoder tokens, got %d' % (self.model.d_in, xs[0].shape[-1]))
        S = self.model.similarity(xs)
        if self.verbose:
            print('retrieval: %d views, %d words, similarity computed on %s' % (len(xs), self.model.k, dev))
        return S.cpu().numpy()
