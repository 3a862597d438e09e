"""The references, the bound and the memory checks of the two image input kernels (tests/input_ref.py, errbound.aa_resize_bound) are SOUND and TIGHT (CPU
only): at the cases and images of tests/test_hip_input.py an fp32 emulation of the correct kernel - the same order of operations, with the accumulations
fused and unfused - stays at <= 0.5 of the bound (and is bit-exact at the identity resize), and each planted wrong kernel exceeds the bound at exactly the
cases its CAUGHT row names: everywhere else it is the same computation as the right kernel, and the row's comment says why.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import errbound as EB
import input_ref as IR
import smallops_ref as SR

F32 = np.float32
FMT16 = {'bf16': torch.bfloat16, 'f16': torch.float16}


# ------------------------------------------------------------------------------------------------------------------------------------------- image_prepare
def emu_axis(n_in, scale, idx, support_unclamped=False, short=False, analytic=False, half=True):
    """aa_window and the normalised tap weights of one axis in numpy fp32, one rounding per operation, the weight sum in the kernel's order.
    -> (lo int64 [n], w fp32 [n, nmax]: zero behind a window's last tap)"""
    scale = F32(scale)
    up = scale < 1 and not support_unclamped
    support = F32(1) if up else scale
    inv = F32(1) if up else F32(1) / scale
    h = F32(0.5) if half else F32(0)
    c = scale * (idx.astype(F32) + h)
    lo = np.maximum((c - support + F32(0.5)).astype(np.int64), 0)
    cnt = np.minimum((c + support + F32(0.5)).astype(np.int64), n_in) - lo - (1 if short else 0)
    nmax = max(int(cnt.max()), 1)
    t = np.zeros((len(idx), nmax), dtype=F32)
    tot = np.zeros(len(idx), dtype=F32)
    for k in range(nmax):
        x = np.abs(((lo + k).astype(F32) - c + h) * inv)
        tk = np.where((x < 1) & (k < cnt), F32(1) - x, F32(0)).astype(F32)
        t[:, k] = tk
        tot = np.where(k < cnt, tot + tk, tot).astype(F32)
    with np.errstate(invalid='ignore', divide='ignore'):
        w = t / (support if analytic else tot[:, None])
    return lo, np.where(np.arange(nmax)[None, :] < cnt[:, None], w, F32(0)).astype(F32)      # an empty window: the loops do not run, the output is 0


def emu_image_prepare(img, Hr, Wr, top, left, H, W, fused=False, exchange=False, swap_crop=False, no_crop=False, div256=False, reverse=False, **axis):
    """image_prepare_kernel in numpy fp32: pixel = ((v / 255) - 0.5) / 0.5; r = sum_k wx_k pixel (per source row), acc = sum_j wy_j r, both sequential from 0;
    fused: each step one fma (the product exact in float64, rounded once)"""
    img = img.numpy()
    Hs, Ws = img.shape[:2]
    sy, sx = F32(Hs) / F32(Hr), F32(Ws) / F32(Wr)
    if exchange:
        sy, sx = sx, sy
    if swap_crop:
        top, left = left, top
    if no_crop:
        top = left = 0
    y0, wy = emu_axis(Hs, sy, np.arange(H) + top, **axis)
    x0, wx = emu_axis(Ws, sx, np.arange(W) + left, **axis)
    P = ((img.astype(F32) / F32(256 if div256 else 255) - F32(0.5)) / F32(0.5)).transpose(2, 0, 1)
    if reverse:
        P = P[::-1]

    def step(acc, w, v):
        if fused:
            return (acc.astype(np.float64) + w.astype(np.float64) * v.astype(np.float64)).astype(F32)
        return acc + (w * v).astype(F32)
    r = np.zeros((3, Hs, W), dtype=F32)
    for k in range(wx.shape[1]):
        r = step(r, wx[None, None, :, k], P[:, :, np.minimum(x0 + k, Ws - 1)])
    acc = np.zeros((3, H, W), dtype=F32)
    for j in range(wy.shape[1]):
        acc = step(acc, wy[None, :, j, None], r[:, np.minimum(y0 + j, Hs - 1), :])
    return torch.from_numpy(acc)


def ratio(got, ref, bound):
    r = (got.double() - ref).abs() / bound
    return float(torch.where(torch.isnan(r), torch.full_like(r, float('inf')), r).max())


_REFS = {}


def reference(case, kind):
    """(image, reference, bound) of a case and image kind, computed once"""
    if (case, kind) not in _REFS:
        Hs, Ws, Hr, Wr, top, left, H, W = IR.IMAGE_CASES[case]
        img = IR.image(kind, case)
        ref = IR.aa_resize(img, Hr, Wr, top, left, H, W)[0]
        _REFS[case, kind] = img, ref, EB.aa_resize_bound(IR.img_norm(img), (Hr, Wr), (top, left, H, W))
    return _REFS[case, kind]


@pytest.mark.parametrize('case', list(IR.IMAGE_CASES))
def test_reference_is_torch_antialias_in_float64(case):
    """input_ref.aa_resize against torch's own float64 antialiased interpolation and a crop (another implementation of the same rule): 1e-12 of the data's
    range of 2; and the conditions each case was built for hold on the reference"""
    Hs, Ws, Hr, Wr, top, left, H, W = IR.IMAGE_CASES[case]
    for kind in IR.IMAGE_KINDS:
        img, ref, _ = reference(case, kind)
        IR.image_conditions(case, kind, ref)
        t = F.interpolate(IR.img_norm(img)[None], size=(Hr, Wr), mode='bilinear', align_corners=False, antialias=True)[0][:, top:top + H, left:left + W]
        assert float((ref - t).abs().max()) <= 2e-12, (kind, float((ref - t).abs().max()))
        if kind in ('zero', 'grey', 'white'):
            v = {'zero': -1.0, 'grey': (128 / 255 - 0.5) / 0.5, 'white': 1.0}[kind]
            assert float((ref - v).abs().max()) <= 1e-15


def test_recipe_cases_are_the_recipe():
    """the eight shapes kept from test_image_prepare_matches_torch_antialias are what resize_recipe makes of them: the centre crop is taken in the source
    (prepare_image uploads only the kept pixels), the kernel resizes the crop with crop origin (0, 0)"""
    from panst3r_amd.engine.images import resize_recipe
    import warnings
    for case, (Hs, Ws, size) in IR.RECIPE_CASES.items():
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            _, (Hc, Wc), (Ho, Wo) = resize_recipe(size, 16, Hs, Ws)
        assert IR.IMAGE_CASES[case] == (Hc, Wc, Ho, Wo, 0, 0, Ho, Wo)


@pytest.mark.parametrize('case', list(IR.IMAGE_CASES))
def test_image_prepare_emulation_meets_the_bound(case):
    """fused and unfused accumulations, every image kind: <= 0.5 of the bound; bit-exact at the identity; the coordinate term is zero exactly where the fp32
    scale, centres and inverse support are exact"""
    Hs, Ws, Hr, Wr, top, left, H, W = IR.IMAGE_CASES[case]
    worst = 0.0
    for kind in IR.IMAGE_KINDS:
        img, ref, bound = reference(case, kind)
        for fused in (False, True):
            got = emu_image_prepare(img, Hr, Wr, top, left, H, W, fused=fused)
            worst = max(worst, ratio(got, ref, bound))
            if case == 'identity':
                assert torch.equal(got, ((img.permute(2, 0, 1).float() / 255.0 - 0.5) / 0.5))
    print('image_prepare emulation %s: largest |err| / bound %.3f, largest bound %.3g' % (case, worst, float(reference(case, 'noise')[2].max())))
    assert worst <= 0.5, worst
    coord = float(EB.aa_axis(Hs, Hr, top, H)['coord'].max() + EB.aa_axis(Ws, Wr, left, W)['coord'].max())
    assert (coord == 0.0) == (case in ('identity', '2to1', '4to1', '96x128')), coord                     # 1 / 40, 1 / 1.5, 1 / 3.125 ... round
    assert coord <= (4e-7 if all(IR.fp32_exact_scale(*a) for a in ((Hs, Hr), (Ws, Wr))) else 1e-3)      # an exact scale leaves only fl(1 / scale)


ALL = set(IR.SMALL_CASES)
CROPPED = {'crop_inside', 'crop_to_the_end', 'tall_window'}
# planted kernel -> (the emulation's switch, the small cases at which it is another computation)
IMAGE_CAUGHT = {
    # support and inv taken as the scale itself: the same expression wherever both scales are >= 1
    'support not clamped when up-scaling': (dict(support_unclamped=True), {'upscale', 'one_source_row', 'tall_window'}),
    # the dropped last tap weighs 0 at the identity - except in the last row and column, whose window is clipped to that one tap
    'window one tap short': (dict(short=True), ALL),
    # sum = support for an unclipped window of an integer ratio; the identity has no clipped window
    'weights over the analytic support': (dict(analytic=True), ALL - {'identity'}),
    # centre scale i, taps at j: at the identity the same differences j - i
    'no half-pixel offset': (dict(half=False), ALL - {'identity'}),
    # the same number where Hs / Hr == Ws / Wr
    'Hs / Hr and Ws / Wr exchanged': (dict(exchange=True), {'upscale', 'crop_inside', 'crop_to_the_end', 'one_source_row', 'tall_window', 'below_one_wave'}),
    'top and left exchanged': (dict(swap_crop=True), CROPPED),
    'crop ignored': (dict(no_crop=True), CROPPED),
    '/ 256 for / 255': (dict(div256=True), ALL),
    'channels reversed': (dict(reverse=True), ALL),
}


@pytest.mark.parametrize('plant', list(IMAGE_CAUGHT))
def test_planted_image_kernels_exceed_the_bound(plant):
    kw, caught = IMAGE_CAUGHT[plant]
    assert caught and caught <= ALL
    seen, rows = set(), []
    for case in IR.SMALL_CASES:
        Hs, Ws, Hr, Wr, top, left, H, W = IR.IMAGE_CASES[case]
        worst = 0.0
        for kind in IR.IMAGE_KINDS:
            img, ref, bound = reference(case, kind)
            worst = max(worst, ratio(emu_image_prepare(img, Hr, Wr, top, left, H, W, **kw), ref, bound))
        rows.append('%s %.3g' % (case, worst))
        assert worst > 1 or worst <= 0.5, (case, worst)          # nothing in between: either another computation or the same one
        if worst > 1:
            seen.add(case)
    print('planted "%s": largest |err| / bound per case: %s' % (plant, ', '.join(rows)))
    assert seen == caught, (sorted(seen - caught), sorted(caught - seen))


def test_planted_image_kernels_on_a_recipe_shape():
    """one of the shapes kept from the earlier test (unequal scales, 273 x 385 after the crop is too much to ask: 500 x 700 at 384): every plant that is
    another computation there exceeds the bound"""
    case = '500x700'
    Hs, Ws, Hr, Wr, top, left, H, W = IR.IMAGE_CASES[case]
    img, ref, bound = reference(case, 'planes')
    for plant, (kw, _) in IMAGE_CAUGHT.items():
        r = ratio(emu_image_prepare(img, Hr, Wr, top, left, H, W, **kw), ref, bound)
        assert (r > 1) == (plant not in ('support not clamped when up-scaling', 'top and left exchanged', 'crop ignored')), (plant, r)


# ------------------------------------------------------------------------------------------------------------------------------------------- patch_rows
def emu_dino_rows(img, transposed, untransposed_read=False, untransposed_grid=False):
    """the DINOv2 half of patch_rows_kernel in numpy fp32, contraction off: per (token, channel, dy, dx) the ImageNet-normalised taps
    ((v 0.5 + 0.5) - mean) / std blended as (a (1 - lx) + b lx) (1 - ly) + (d (1 - lx) + e lx) ly -> fp32 [n T, K_DINO]"""
    im = img.numpy()
    n, _, H, W = im.shape
    pe, pd = IR.P_ENC, IR.P_DINO
    gh, gw = H // pe, W // pe
    T = gh * gw
    Hd, Wd = (W, H) if transposed else (H, W)
    ghd, gwd = Hd // pe, Wd // pe
    sy, sx = F32(Hd) / F32(ghd * pd), F32(Wd) / F32(gwd * pd)
    t = np.arange(T)
    ty, tx = (t // gw, t % gw) if untransposed_grid else (t // gwd, t % gwd)

    def coords(tok, s, size):
        o = (tok[:, None] * pd + np.arange(pd)[None, :]).astype(F32)
        f = np.maximum((o + F32(0.5)) * s - F32(0.5), F32(0)).astype(F32)
        i0 = f.astype(np.int64)
        return i0, np.minimum(i0 + 1, size - 1), (f - i0.astype(F32)).astype(F32)
    y0, y1, ly = (a[:, :, None] for a in coords(ty, sy, Hd))                 # [T, pd, 1]
    x0, x1, lx = (a[:, None, :] for a in coords(tx, sx, Wd))                 # [T, 1, pd]
    mean = np.asarray(SR.IMAGENET_MEAN, dtype=F32)[None, :, None]
    std = np.asarray(SR.IMAGENET_STD, dtype=F32)[None, :, None]
    flat = im.reshape(n, 3, H * W)
    nv = (((flat * F32(0.5) + F32(0.5)) - mean) / std).astype(F32)

    def px(y, x):
        idx = (x * W + y) if (transposed and not untransposed_read) else (y * W + x)
        return nv[:, :, np.minimum(idx, H * W - 1)]                          # [n, 3, T, pd, pd]
    one = F32(1)
    topv = px(y0, x0) * (one - lx) + px(y0, x1) * lx
    botv = px(y1, x0) * (one - lx) + px(y1, x1) * lx
    val = (topv * (one - ly) + botv * ly).astype(F32)
    return torch.from_numpy(val.transpose(0, 2, 1, 3, 4).reshape(n * T, IR.K_DINO))


def emu_patch_rows(img, bufs, transposed, vec, pairs, plant=None):
    """patch_rows_kernel into the operand views of `bufs`: the same values on every path, stored as whole 16-element runs (vec), as pairs (pairs) or one by
    one; the row's padding thread zero-fills columns K .. ld - 1"""
    fmt = bufs['enc'][1].dtype
    rows = {'enc': SR.patchify(img, IR.P_ENC, torch.float32),
            'dino': emu_dino_rows(img, transposed, untransposed_read=plant == 'untransposed read', untransposed_grid=plant == 'untransposed grid')}
    for name, K in (('enc', IR.K_ENC), ('dino', IR.K_DINO)):
        store, view = bufs[name]
        nrows, ld = view.shape
        first = (view.data_ptr() - store.data_ptr()) // store.element_size()
        if plant != 'padding not zeroed':
            for r in range(nrows):
                store[first + r * ld + K:first + (r + 1) * ld + (1 if plant == 'padding one too far' else 0)] = 0
        v = rows[name].to(fmt)
        if name == 'dino' and pairs and plant == 'pair halves exchanged':
            v = v.view(nrows, K // 2, 2).flip(-1).reshape(nrows, K)
        if (name == 'enc' and vec) or (name == 'dino' and pairs):
            w = 16 if name == 'enc' else 2
            for c0 in range(0, K, w):
                view[:, c0:c0 + w] = v[:, c0:c0 + w]
        else:
            for c0 in range(K):
                view[:, c0] = v[:, c0]


TRANSPOSED = {(l, s) for l in IR.PATCH_LAYOUTS for s in IR.PATCH_SHAPES if s[2]}
EVERY = {(l, s) for l in IR.PATCH_LAYOUTS for s in IR.PATCH_SHAPES}
# planted kernel -> the (layout, shape) at which the checker must refuse it
PATCH_CAUGHT = {
    'padding not zeroed': EVERY,                                                            # every layout pads at least one of the two outputs
    'padding one too far': EVERY,                                                           # the last row's zero lands in the guard row behind it
    'pair halves exchanged': {(l, s) for l, s in EVERY if l not in ('ld_dino_589', 'dino_offset')},     # the single-store layouts make no pairs
    'untransposed read': TRANSPOSED,
    'untransposed grid': TRANSPOSED,
}


@pytest.mark.parametrize('fmt', list(FMT16))
@pytest.mark.parametrize('layout', list(IR.PATCH_LAYOUTS))
def test_patch_rows_emulation_and_planted_kernels(layout, fmt):
    """the emulation passes the checker of the GPU test at every layout and shape with the DINOv2 half at <= 0.5 of its bound; every planted kernel is
    refused at exactly the cases of its PATCH_CAUGHT row"""
    f = FMT16[fmt]
    for shape in IR.PATCH_SHAPES:
        H, W, transposed = shape
        T = (H // IR.P_ENC) * (W // IR.P_ENC)
        img = IR.patch_image(H, W, layout)
        enc_ref, dino_ref, dino_bound = IR.patch_refs(img, transposed, f)
        assert PATCH_THREADS(T) == 1104 and PATCH_THREADS(T) % 256 != 0

        def run(plant):
            bufs = IR.patch_buffers(layout, T, f)
            vec, pairs = IR.patch_branches(layout, bufs['enc'][1].data_ptr(), img.data_ptr(), bufs['dino'][1].data_ptr())
            emu_patch_rows(img, bufs, transposed, vec, pairs, plant)
            return IR.check_patch_buffers(bufs, enc_ref, dino_ref, dino_bound, '%s %s' % (layout, shape))
        r = run(None)
        assert r <= 0.5, r
        for plant, caught in PATCH_CAUGHT.items():
            if (layout, shape) in caught:
                with pytest.raises(AssertionError):
                    run(plant)
            else:
                assert run(plant) <= 0.5, plant


def PATCH_THREADS(T):
    return IR.PATCH_N * T * (3 * IR.P_ENC + 1 + 3 * IR.P_DINO + 1)


def test_patch_layouts_cover_the_issue():
    assert set(PATCH_CAUGHT) == {'padding not zeroed', 'padding one too far', 'pair halves exchanged', 'untransposed read', 'untransposed grid'}
    assert all(v for v in PATCH_CAUGHT.values())
    L = IR.PATCH_LAYOUTS
    assert L['ld_enc_772']['ld_enc'] & 7 and not L['padded_enc']['ld_enc'] & 7 and L['padded_enc']['ld_dino'] == IR.K_DINO and L['ld_dino_589']['ld_dino'] & 1


def test_the_two_wrappers_refuse_without_assert():
    """`python -O` removes assert statements: the operand checks of hip.image_prepare and hip.patch_rows must not be made of them (what they refuse is
    tests/test_hip_input.py's to show)"""
    import ast
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'panst3r_amd', 'hip.py')
    with open(path) as f:
        tree = ast.parse(f.read())
    fns = {n.name: n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name in ('image_prepare', 'patch_rows')}
    assert set(fns) == {'image_prepare', 'patch_rows'}
    for name, fn in fns.items():
        assert not [n for n in ast.walk(fn) if isinstance(n, ast.Assert)], name
        called = {n.func.id for n in ast.walk(fn) if isinstance(n, ast.Call) and isinstance(n.func, ast.Name)}
        assert '_Operands' in called and '_rowmajor' not in called, (name, sorted(called))          # _rowmajor asserts
