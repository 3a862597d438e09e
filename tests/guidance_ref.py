"""A plain restatement of LoftUp's guidance front end (csrc/loftup.hip: 2x2 mean, MinMaxScaler, Fourier features, the low-resolution positional features)
in numpy on the CPU, one fp32 rounding per torch operation, which returns the INTERMEDIATE values - the down-sampled image, the scaled colours, the fp32 phases -
that oracle/panoptic.py keeps inside its modules.  tests/test_guidance_host.py holds it to torch bit for bit; tests/test_hip_guidance.py holds the kernels to
float64 sin / cos of ITS fp32 phases under errbound.guidance_bound.

numpy's float32 arithmetic rounds every operation once (IEEE), so a chain of numpy operations is the chain of torch operations.  numpy has no fp32 fma: where
torch uses one (linspace), the product and the sum are taken in float64 and rounded once - exact, because a 24-bit by 24-bit product has 48 bits and stays
exact in float64, and so does its sum with a 24-bit addend of comparable magnitude.

Three switches plant the mistakes the comparison exists to catch (tests/test_guidance_host.py): `serial` (the 2x2 mean summed ((a + b) + c) + d),
`mirrored=False` (linspace as a + i step throughout), `fused` (the phase coordinate * frequency + bias with ONE rounding)."""
import numpy as np
import torch

F32, F64 = np.float32, np.float64


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def half_mean(img, serial=False):
    """0.25 ((a00 + a01) + (a10 + a11)) in fp32: torch's bilinear x0.5 (align_corners=False), row sums first.  img [..., H, W] -> [..., H / 2, W / 2]"""
    a = _np(img).astype(F32)
    a00, a01, a10, a11 = a[..., 0::2, 0::2], a[..., 0::2, 1::2], a[..., 1::2, 0::2], a[..., 1::2, 1::2]
    if serial:
        return F32(0.25) * (((a00 + a01) + a10) + a11)
    return F32(0.25) * ((a00 + a01) + (a10 + a11))


def linspace32(a, b, n, mirrored=True):
    """torch.linspace(a, b, n) in fp32: step = (b - a) / (n - 1), fma(step, i, a) below the middle, fma(-step, n - 1 - i, b) from it on"""
    a, b = F32(a), F32(b)
    if n <= 1:
        return np.full(max(n, 0), a, F32)
    step = F64((b - a) / F32(n - 1))
    i = np.arange(n, dtype=F64)
    lo = (step * i + F64(a)).astype(F32)
    if not mirrored:
        return lo
    hi = (-step * (n - 1 - i) + F64(b)).astype(F32)
    return np.where(i < n // 2, lo, hi)


def freqs32(nf, mirrored=True):
    """exp(linspace(-2, 10, nf)) correctly rounded: exp in float64 of the fp32 abscissa, rounded once"""
    return np.exp(linspace32(-2, 10, nf, mirrored).astype(F64)).astype(F32)


def minmax(img2):
    """per (view, channel) (min, max) of the down-sampled image [n, 3, H2, W2] -> [n, 3, 2]"""
    return np.stack([img2.min(axis=(2, 3)), img2.max(axis=(2, 3))], -1)


def scaled(img2, lo, hi):
    """MinMaxScaler: (x - lo) / max(hi - lo, 1e-4) - 0.5, each operation in fp32; lo / hi broadcast against img2 ([n, 3, 1, 1] for a table per view)"""
    img2, lo, hi = (np.asarray(t, F32) for t in (img2, lo, hi))
    return (img2 - lo) / np.maximum(hi - lo, F32(1e-4)) - F32(0.5)


def phases(base, biases, nf, fused=False, mirrored=True):
    """the fp32 arguments of sin and of cos.  base [n, dm, h, w] (y grid, x grid, then the scaled colours), biases [2, dm, nf] whose storage is READ as
    [2][nf * dm] (index f * dm + d: a reshape, not a transpose).  phase = round(round(base * frequency) + bias): two torch operations, two roundings.
    Returns (s_in, c_in), each pixel-major [n, h w, nf dm] with channel f * dm + d."""
    base = np.asarray(base, F32)
    n, dm, h, w = base.shape
    fr = freqs32(nf, mirrored)
    bs = _np(biases).astype(F32).reshape(2, nf, dm)
    pm = base.reshape(n, dm, h * w).transpose(0, 2, 1)[:, :, None, :]                    # [n, P, 1, dm]
    out = []
    for k in range(2):
        if fused:
            ph = (pm.astype(F64) * fr.astype(F64)[None, None, :, None] + bs[k].astype(F64)[None, None]).astype(F32)
        else:
            ph = pm * fr[None, None, :, None] + bs[k][None, None]
        out.append(ph.reshape(n, h * w, nf * dm))
    return out[0], out[1]


def grid(n, h, w, mirrored=True):
    """[n, 2, h, w]: linspace(-1, 1, h) down the rows, linspace(-1, 1, w) along them"""
    gy, gx = linspace32(-1, 1, h, mirrored), linspace32(-1, 1, w, mirrored)
    g = np.stack([np.broadcast_to(gy[:, None], (h, w)), np.broadcast_to(gx[None, :], (h, w))])
    return np.broadcast_to(g[None], (n, 2, h, w)).astype(F32)


def guidance_inputs(img, biases, nf, mm=None, serial=False, fused=False, mirrored=True):
    """everything up to the sin / cos of pst_loftup_guidance_gn: img [n, 3, H, W] fp32, mm None (a table per view) or [n, 3, 2].
    Returns dict(img2, mm, col [n, P, 3], s_in, c_in [n, P, 5 nf])."""
    img2 = half_mean(img, serial)
    n, _, h, w = img2.shape
    own = minmax(img2)
    tab = own if mm is None else _np(mm).astype(F32)
    col = scaled(img2, tab[:, :, 0, None, None], tab[:, :, 1, None, None])
    base = np.concatenate([grid(n, h, w, mirrored), col], 1)
    s_in, c_in = phases(base, biases, nf, fused, mirrored)
    return dict(img2=img2, mm=own, col=col.reshape(n, 3, h * w).transpose(0, 2, 1), s_in=s_in, c_in=c_in)


def lr_pe_inputs(biases, n, h, w, nf=5):
    """the positional features of the token grid: no colours, dm = 2 -> s_in, c_in [n, h w, 2 nf]"""
    return phases(grid(n, h, w), biases, nf)


def features64(s_in, c_in, col=None):
    """sin / cos in float64 of the fp32 phases; channels [sin | cos | colours] -> float64 torch [n, P, CH]"""
    parts = [np.sin(s_in.astype(F64)), np.cos(c_in.astype(F64))] + ([col.astype(F64)] if col is not None else [])
    return torch.from_numpy(np.concatenate(parts, -1))


def features32(s_in, c_in, col=None):
    """torch.sin / torch.cos of the fp32 phases -> fp32 torch [n, P, CH]: what the oracle module computes"""
    parts = [torch.sin(torch.from_numpy(np.ascontiguousarray(s_in))), torch.cos(torch.from_numpy(np.ascontiguousarray(c_in)))]
    if col is not None:
        parts.append(torch.from_numpy(np.ascontiguousarray(col)))
    return torch.cat(parts, -1)


# ------------------------------------------------------------------------------------------------------------------------------------------- cases
# (H, W, n) of the full-resolution image and what the shape reaches in csrc/loftup.hip; P = (H / 2) (W / 2) output pixels per view
SHAPES = [
    (132, 250, 3),      # P = 8250, 129 tiles: the stats pass strides once, its second trip is the ragged tile of 58 pixels; down2_minmax loops 9 times; odd W2
    (2, 250, 2),        # P = 125: H2 = 1, the n = 1 branch of linspace
    (2, 6, 1),          # P = 3: one tile, 61 idle lanes clamped to pixel P - 1
    (384, 4, 1),        # P = 384: linspace at n = 192
    (4, 512, 1),        # P = 512: linspace at n = 256
    (16, 24, 2),        # P = 96: the case of tests/test_hip_ops.py
]
NF = 20
RANGE = F32(1e-4)                                   # MinMaxScaler's clamp
BELOW = np.nextafter(RANGE, F32(0))                 # a float32 below it


def shape_id(s):
    return '%dx%dx%d' % s


def max_index(P):
    """where the cases put a plane's maximum: inside the last, partial trip of down2_minmax_kernel's 1024-thread loop and not at its last pixel"""
    first = (P - 1) // 1024 * 1024                   # the first pixel of the last trip
    assert first < P - 1
    return first + (P - 1 - first) // 2


def make_case(H, W, n, seed=0, nf=NF):
    """inputs built to decide.  Every view differs.  Every plane's minimum of the down-sampled image sits at its last pixel and its maximum at max_index(P)
    (both as 2x2 blocks of one value, whose mean is that value exactly).  Special planes: `const` is constant (range 0: the 1e-4 clamp applies), `exact` has
    a range of exactly float32(1e-4), `below` a range one float32 below it.  With n >= 2 they are the three planes of view 0, with n = 1 planes 2 and 1
    (`exact` is left out: plane 0 stays an ordinary one).  Returns dict(img [n, 3, H, W], biases [2, 5, nf], gamma, beta [10 nf + 3], special, scope)."""
    g = np.random.Generator(np.random.PCG64(1000 + seed))
    H2, W2 = H // 2, W // 2
    P = H2 * W2
    img = np.clip(g.standard_normal((n, 3, H, W)) * (0.25 + 0.1 * np.arange(n))[:, None, None, None], -0.8, 0.8).astype(F32)
    special = {(0, 0): 'const', (0, 1): 'exact', (0, 2): 'below'} if n >= 2 else {(0, 2): 'const', (0, 1): 'below'}
    ilo, ihi = P - 1, max_index(P)

    def put(v, c, idx, val):
        y, x = divmod(idx, W2)
        img[v, c, 2 * y:2 * y + 2, 2 * x:2 * x + 2] = val
    for v in range(n):
        for c in range(3):
            kind = special.get((v, c))
            if kind == 'const':
                img[v, c] = F32(0.25)
                continue
            if kind:
                top = RANGE if kind == 'exact' else BELOW
                img[v, c] = g.uniform(0.1e-4, 0.9e-4, (H, W)).astype(F32)
                lo, hi = F32(0), top
            else:
                lo, hi = F32(-0.9 - 0.01 * (3 * v + c)), F32(0.9 + 0.005 * (3 * v + c))
            put(v, c, ihi, hi)
            put(v, c, ilo, lo)
    return dict(img=torch.from_numpy(img), biases=torch.from_numpy(g.standard_normal((2, 5, nf)).astype(F32)),
                gamma=torch.from_numpy((1 + 0.1 * g.standard_normal(10 * nf + 3)).astype(F32)),
                beta=torch.from_numpy((0.1 * g.standard_normal(10 * nf + 3)).astype(F32)), special=special,
                scope=[0, 1, 0][:n] if n == 3 else [0] * n, ilo=ilo, ihi=ihi)


def pooled(mm, scope):
    """pst_minmax_merge on the host: [n, 3, 2] -> per view the (min, max) over the views of its scope"""
    out = np.empty_like(mm)
    for v, s in enumerate(scope):
        grp = [u for u, t in enumerate(scope) if t == s]
        out[v, :, 0], out[v, :, 1] = mm[grp][:, :, 0].min(0), mm[grp][:, :, 1].max(0)
    return out


def assert_case(case, r):
    """the properties the case was built for, on the restatement r = guidance_inputs(case['img'], ...) with a table per view"""
    img2, mm = r['img2'], r['mm']
    n, _, H2, W2 = img2.shape
    flat = img2.reshape(n, 3, -1)
    for v in range(n):
        for c in range(3):
            kind = case['special'].get((v, c))
            rng = mm[v, c, 1] - mm[v, c, 0]
            if kind == 'const':
                assert rng == 0 and (flat[v, c] == flat[v, c, 0]).all()
                continue
            assert flat[v, c].argmin() == case['ilo'] and (flat[v, c] == mm[v, c, 0]).sum() == 1, (v, c)
            assert flat[v, c].argmax() == case['ihi'] and (flat[v, c] == mm[v, c, 1]).sum() == 1, (v, c)
            if kind == 'exact':
                assert rng == RANGE
            elif kind == 'below':
                assert rng == BELOW and rng < RANGE
            else:
                assert rng > 1
    for v in range(1, n):
        assert not np.array_equal(img2[0], img2[v])
