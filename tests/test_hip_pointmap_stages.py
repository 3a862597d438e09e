"""Stage-level parity of csrc/pointmap.hip: pointmap_activate, focal_weiszfeld and rigid_moments called directly and compared with float64 references
(tests/pp_stage_cases.py) under per-element bounds (tests/errbound.py: activate_bound, conf_bound, moments_bound; the focal bound is built per input).

pointmap_activate: exact zero vectors and |xyz| of 1e-12, 1e-9, 1e-4 (the max(d, 1e-8) branch and the small-argument branch of expm1), |xyz| up to 88 (the
largest whose fp32 result is finite), confidence logits from -30 to 80, npix up to 12 x 384 x 512 (more than 8192 x 256 threads: the grid-stride loop
wraps); 'linear' copies bits.  The allowances of the device expf / expm1f are measured (errbound.EXPF_ULP / EXPM1F_ULP; test_device_math_ulps logs them).

focal_weiszfeld: fewer pixels than threads and sizes that are no multiple of 1024; iters 0 (the closed-form L2 start), 1, 10; a principal point per view;
points with z == 0, x == z == 0 and denormal z contribute nothing; 10 % outliers.  The kernel keeps f, residuals and weights in fp32 and only the sums in
double, and the error of a step feeds the next one, so the bound is built by pp_stage_cases.ref_focal: the first-order bound of one step (every fp32 rounding
of u, w, the residual, the root and the weight; a weight's error multiplies ta - f' tb) and per step B <- L B + step bound, L the Lipschitz factor of the
float64 step on that input by a finite difference.  The step bound is STATISTICAL, not worst-case: the roundings of different pixels are independent, and
their sum is bounded by its 5-sigma envelope (errbound.LAMBDA) where that is below the worst case, which would be sqrt(P) times the real error and hide a
wrong weight rule.  Resulting bound on the MI355X cases: at most 5.8e-6 of f,
Lipschitz factors up to 1.37; largest observed error / bound 0.25 (profiles/output_kernel_margins.jsonl).

rigid_moments: all 16 numbers against float64 numpy, bound n 2^-53 sum |terms| plus the fp32 rounding of conf + weight_offset; offsets 0 and -1, mixed signs.
Every stage runs twice (equal bits) and once through torch.ops.panst3r_hip.
Largest observed error / bound: pts3d 0.32, conf 0.50 (the rounding of 1 + e where e is below an ulp of 1), moments 0.44 with offset 0 (double arithmetic only) and 0.50 with offset -1
(the rounding of conf - 1, allowed twice).  38 tests, 4 s."""
import json
import os

import numpy as np
import pytest
import torch

import errbound as EB
import pp_stage_cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CANARY = -777.0


def _log(**kw):
    if os.environ.get('PST_STAGE_LOG'):
        with open(os.environ['PST_STAGE_LOG'], 'a') as f:
            f.write(json.dumps(kw) + '\n')


def _hip():
    from panst3r_amd import hip
    import panst3r_amd.ops                  # noqa: F401
    return hip


def _activate(hip, raw_d, mode, via_ops=False):
    n = raw_d.shape[0]
    pts, loc, conf = (torch.full(s, CANARY, device=DEV) for s in ((n, 3), (n, 3), (n,)))
    (torch.ops.panst3r_hip.pointmap_activate if via_ops else hip.pointmap_activate)(raw_d, pts, loc, conf, mode)
    torch.cuda.synchronize()
    return pts.cpu(), loc.cpu(), conf.cpu()


@pytest.mark.parametrize('npix', C.ACT_NPIX)
def test_pointmap_activate(npix):
    hip = _hip()
    raw = C.activate_case(npix, 0)
    rd = raw.to(DEV)
    got = _activate(hip, rd, 0)
    for again in (_activate(hip, rd, 0), _activate(hip, rd, 0, via_ops=True)):
        assert all(torch.equal(a, b) for a, b in zip(got, again))
    p, l, c, bp, bl, bc = C.ref_activate(raw)
    ratios = [EB.check(g, r, b, 'pointmap_activate %s npix=%d' % (k, npix)) for g, r, b, k in zip(got, (p, l, c), (bp, bl, bc), ('pts3d', 'pts3d_local', 'conf'))]
    lin = _activate(hip, rd, 1)
    assert torch.equal(lin[0], raw[:, 0:3]) and torch.equal(lin[1], raw[:, 3:6]) and torch.equal(lin[2], got[2]), "'linear' must copy bits"
    _log(stage='pointmap_activate', npix=npix, ratio_pts=max(ratios[:2]), ratio_conf=ratios[2])


def test_device_math_ulps():
    """the measurement behind errbound.EXPF_ULP / EXPM1F_ULP: the largest error, in ulps of the exact value, of 1 + expf(c) over c in [0, 80] and of
    x expm1f(d) / d on axis-aligned vectors over d in [1e-12, 88], against float64; the allowances are twice these and the test holds them to that"""
    hip = _hip()
    n = 131072
    raw = torch.zeros(n, 7, dtype=torch.float64)
    raw[:, 6] = torch.cat([torch.linspace(0, 80, n // 2, dtype=torch.float64), torch.logspace(-6, float(np.log10(80.0)), n // 2, dtype=torch.float64)])
    d = torch.cat([torch.logspace(-12, float(np.log10(88.0)), n // 2, dtype=torch.float64), torch.linspace(1e-3, 88.0, n // 2, dtype=torch.float64)])
    raw[:, 0] = d
    raw[:, 4] = -d
    raw = raw.float()
    pts, loc, conf = _activate(hip, raw.to(DEV), 0)
    c64, d64 = raw[:, 6].double(), raw[:, 0].double()
    ulp = lambda v: 2.0 ** (torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126))) - 23)
    e_exp = float(((conf.double() - (1 + c64.exp())).abs() / ulp(c64.exp())).max())
    ref = d64 / d64.clamp_min(1e-8) * torch.expm1(d64)
    e_m1 = float(torch.maximum((pts[:, 0].double() - ref).abs() / ulp(ref), (loc[:, 1].double() + ref).abs() / ulp(ref)).max())
    _log(stage='expf_ulp', observed=e_exp, allowance=EB.EXPF_ULP)
    _log(stage='expm1f_ulp', observed=e_m1, allowance=EB.EXPM1F_ULP)
    print('expf %.3f ulp, expm1f chain %.3f ulp' % (e_exp, e_m1))
    assert 2 * e_exp <= EB.EXPF_ULP and 2 * e_m1 <= EB.EXPM1F_ULP, (e_exp, e_m1)


@pytest.mark.parametrize('iters', C.FOCAL_ITERS)
@pytest.mark.parametrize('H,W', C.FOCAL_HW)
def test_focal_weiszfeld(H, W, iters):
    hip = _hip()
    V = 3
    loc, pp = C.focal_case(H, W, V, 0)
    f_ref, bound, L = C.ref_focal(loc, pp, H, W, iters)
    outs = []
    for via_ops in (False, False, True):
        f = torch.full((V,), CANARY, device=DEV)
        (torch.ops.panst3r_hip.focal_weiszfeld if via_ops else hip.focal_weiszfeld)(loc.to(DEV), pp.to(DEV), f, H, W, iters)
        torch.cuda.synchronize()
        outs.append(f.cpu())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    r = EB.check(outs[0], f_ref, bound, 'focal_weiszfeld %dx%d iters=%d' % (H, W, iters))
    _log(stage='focal_weiszfeld', H=H, W=W, iters=iters, ratio=r, bound_rel=float((bound / f_ref.abs()).max()), lipschitz=L)


@pytest.mark.parametrize('off', [0.0, -1.0])
@pytest.mark.parametrize('V', C.MOMENT_V)
@pytest.mark.parametrize('P', C.MOMENT_P)
def test_rigid_moments(P, V, off):
    hip = _hip()
    x, y, conf = C.moments_case(V, P, 0)
    ref, bound = C.ref_moments(x, y, conf, off)
    outs = []
    for via_ops in (False, False, True):
        out = torch.full((V, 16), CANARY, dtype=torch.float64, device=DEV)
        (torch.ops.panst3r_hip.rigid_moments if via_ops else hip.rigid_moments)(x.to(DEV), y.to(DEV), conf.to(DEV), out, off)
        torch.cuda.synchronize()
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    r = EB.check(outs[0], ref, bound, 'rigid_moments V=%d P=%d off=%g' % (V, P, off))
    _log(stage='rigid_moments', V=V, P=P, off=off, ratio=r)
