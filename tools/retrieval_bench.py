#!/usr/bin/env python
"""Time keyframe retrieval (model/retrieval.py + csrc/retrieval.hip) per step at 50 and 200 views of T = 768 tokens, with seeded weights of ASSUMED
sizes (the checkpoint's are not known here): Denc = D = 1024, whiteners on both sides and a single-Linear projector, k = 65 536 words, nfeat = 300,
multiple assignment 5 / 1.  The must3r encoder pass that produces the tokens (384 x 512 views, fp16) is timed separately: on the use_retrieval path the
scene runner encodes again.  Yardstick: the assignment in ATen on the same GPU (torch.cdist + topk, fp32).  The assign kernel is reported as a fraction
of the 16-bit MFMA peak, counting issued work as 3 x 2 n k D.     python tools/retrieval_bench.py [reps] > profiles/retrieval_bench.json"""
import json
import os
import sys
from argparse import Namespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from panst3r_amd import hip                                                   # noqa: E402
from panst3r_amd.model.retrieval import RetrievalASMK                         # noqa: E402
from panst3r_amd.panst3r import CONFIG_V1, build_from_config                  # noqa: E402
from panst3r_amd.synthetic import fill_module_, synth_image                   # noqa: E402

PEAK16 = 2.5e15          # dense f16 MFMA FLOP/s of an MI355X
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
DEV = torch.device('cuda:0')
DENC, D, K, NFEAT, T, H, W = 1024, 1024, 65536, 300, 768, 384, 512


def seeded_dict(seed=0):
    g = torch.Generator().manual_seed(seed)
    q = lambda n: torch.linalg.qr(torch.randn(n, n, generator=g, dtype=torch.float64))[0]
    sd = {'prewhiten.m': torch.randn(1, DENC, generator=g, dtype=torch.float64) * 0.1, 'prewhiten.p': q(DENC),
          'projector.0.weight': torch.randn(D, DENC, generator=g) / DENC ** 0.5, 'projector.0.bias': torch.randn(D, generator=g) * 0.1,
          'postwhiten.m': torch.randn(1, D, generator=g, dtype=torch.float64) * 0.1, 'postwhiten.p': q(D)}
    cent = torch.randn(K, D, generator=g)
    cent /= cent.norm(dim=1, keepdim=True)
    args = Namespace(prewhiten=True, hdims='', residual=False, postwhiten=True, featweights='l2norm', nfeat=NFEAT, imsize=512, freeze_backbone=True)
    return dict(args=args, model=sd, asmk_codebook={'centroids': cent}, asmk_params={})


def timed(fn, reps=REPS):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), out


def main():
    r = RetrievalASMK(seeded_dict())
    r.packed(DEV)
    model = build_from_config(CONFIG_V1).eval()
    enc = model.must3r_encoder
    fill_module_(enc, seed=1)
    enc.to(DEV)
    model.must3r_encoder = enc
    results = []
    for V in (50, 200):
        imgs = [synth_image(i, H, W).to(DEV) for i in range(V)]
        ts = torch.tensor([[H, W]] * V)
        enc_ms, (xs, _) = timed(lambda: model.forward_must3r_encoder(imgs, ts, amp='fp16'))
        xs = [x.float() for x in xs]
        assert xs[0].shape == (T, DENC), xs[0].shape
        x_all = torch.cat(xs, 0)
        st = {}
        st['head'], feat = timed(lambda: r.head(x_all))
        counts = [min(NFEAT, T)] * V
        in_off = torch.arange(0, (V + 1) * T, T, dtype=torch.int32, device=DEV)
        out_off = torch.arange(0, (V + 1) * counts[0], counts[0], dtype=torch.int32, device=DEV)
        desc = torch.empty(sum(counts), D, dtype=torch.float32, device=DEV)
        st['select'], _ = timed(lambda: hip.retrieval_select(feat, in_off, out_off, desc, T))
        pk = r.packed(DEV)
        st['split'], x3 = timed(lambda: hip.split_operand(desc, 0, kpad=pk['c3'].shape[1] // 3))
        n, m = desc.shape[0], 5
        ids = torch.empty(n, m, dtype=torch.int32, device=DEV)
        dist = torch.empty(n, m, dtype=torch.float32, device=DEV)
        st['assign'], _ = timed(lambda: hip.retrieval_assign(x3, pk['c3'], pk['cnorm'], m, ids, dist))
        view = torch.arange(V, device=DEV).repeat_interleave(counts[0])
        st['group_glue'], (qg, dbg) = timed(lambda: (r.groups(ids, view, 5, V), r.groups(ids, view, 1, V)))
        st['aggregate'], (qb, dbb) = timed(lambda: (r.aggregate(desc, qg)[0], r.aggregate(desc, dbg)[0]))
        st['scores'], _ = timed(lambda: r.scores(qg, qb, dbg, dbb))
        total_ms, _ = timed(lambda: r.similarity(xs))
        aten_ms, (aval, aidx) = timed(lambda: torch.topk(torch.cdist(desc, pk['cent']), m, dim=1, largest=False))
        agree = float((aidx[:, 0].int() == ids[:, 0]).float().mean())
        issued = 3 * 2.0 * n * K * D
        results.append(dict(views=V, tokens_per_view=T, n_desc=n, k=K, D=D, nfeat=NFEAT, ma_q=5, ma_db=1, encoder_ms=enc_ms, retrieval_ms=total_ms,
                            steps_ms=st, assign_nsplit=hip.retrieval_nsplit(n, K), assign_issued_tflops=issued / st['assign'] / 1e9,
                            assign_frac_of_f16_peak=issued / (st['assign'] * 1e-3) / PEAK16, aten_cdist_topk_ms=aten_ms,
                            aten_top1_agreement=agree))
        print(json.dumps(results[-1]), file=sys.stderr, flush=True)
        del xs, x_all, feat, desc, x3
        torch.cuda.empty_cache()
    print(json.dumps(dict(tool='retrieval_bench', assumed_sizes=True, peak16_flops=PEAK16, reps=REPS, results=results), indent=1))


if __name__ == '__main__':
    main()
