"""Plain float64 / exact restatements of the small row and pixel operations at the bottom of csrc/misc.hip and in csrc/text.hip, written from the header's
description (include/panst3r_hip.h) and the oracle's expressions, not from the kernels: l2norm_rows, resize_bilinear, dino_preprocess (float64 references,
held under the bounds of tests/errbound.py) and mean4, add_cast, patchify, token_embed, attn_mask_from_logits (fixed fp32 expressions, compared exactly).

tests/test_smallops_host.py proves on the CPU that an fp32 emulation of each kernel meets its bound and that the planted mistakes fail it;
tests/test_hip_smallops.py holds the kernels to the same references at the same shapes (the case generators below are shared by both).
"""
import numpy as np
import torch
import torch.nn.functional as F

F32 = np.float32
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def rn(seed, *shape, scale=1.0):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32))


# ------------------------------------------------------------------------------------------------------------------------------------------- l2norm_rows
def l2norm(x, eps):
    """x / (||x||_2 + eps) per row, the norm in float64 of the fp32 inputs (an all-zero row with eps = 0 is 0 / 0 = NaN, as in the expression)"""
    x64 = x.double()
    return x64 / (x64.norm(dim=-1, keepdim=True) + float(F32(eps)))


L2_D = (1, 48, 64, 65, 128, 200, 768, 1152)
L2_ROWS = (1, 3, 4, 5, 257)


def l2norm_case(rows, D, seed=0):
    """fp32 rows for l2norm_rows.  Columns from 64 on carry three times the weight of the first 64: with N(0, 1) columns throughout, a kernel that stops after
    column 63 of a 65-wide row moves the norm by about 1 / 130, which the bf16 output rounding (2 x 2^-8) hides.  rows >= 3: row 1 is quiet (norm about 1e-6,
    where eps = 1e-7 moves the result by 10 %), row 2 has one element of 1e18 (its square is finite in fp32); rows >= 5: row 4 is all zero; the last row of
    257 (alone in its block) is quiet too.  A single row (rows == 1) is quiet: the only row that tells where eps is added."""
    x = rn(1000 + 7 * rows + D + seed, rows, D)
    x[:, 64:] *= 3.0
    quiet = [0] if rows == 1 else ([1] if rows < 257 else [1, 256])
    for r in quiet:
        x[r] *= 1e-6 / float(x[r].double().norm())
    if rows >= 3:
        x[2, (D - 1) // 2] = 1e18
    if rows >= 5:
        x[4] = 0.0
    return x


# ------------------------------------------------------------------------------------------------------------------------------------------- bilinear resize
def source_coords(S, Dn):
    """the header's rule in fp32, one rounding per operation: src = max((dst + 0.5) * (S / D) - 0.5, 0); taps floor(src) (never beyond S - 1) and
    min(floor(src) + 1, S - 1); weight src - floor(src) (exact).  The coordinate is fp32 because it decides the taps: a float64 coordinate can floor
    differently at an exact integer.  -> (i0 int64, i1 int64, w float64, src float64), each [Dn]"""
    s = F32(S) / F32(Dn)
    f = np.maximum((np.arange(Dn, dtype=F32) + F32(0.5)) * s - F32(0.5), F32(0.0)).astype(F32)
    i0 = np.minimum(np.floor(f).astype(np.int64), S - 1)
    i1 = np.minimum(i0 + 1, S - 1)
    w = (f - i0.astype(F32)).astype(np.float64)
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(w), torch.from_numpy(f.astype(np.float64))


def blend(src, Hd, Wd):
    """4-tap blend in float64 of src [..., Hs, Ws] at the fp32 source coordinates.  -> (out [..., Hd, Wd], max |tap| [..., Hd, Wd], fy [Hd, 1], fx [1, Wd])"""
    s = src.double()
    y0, y1, wy, fy = source_coords(s.shape[-2], Hd)
    x0, x1, wx, fx = source_coords(s.shape[-1], Wd)
    r0, r1 = s.index_select(-2, y0), s.index_select(-2, y1)
    a, b, d, e = r0.index_select(-1, x0), r0.index_select(-1, x1), r1.index_select(-1, x0), r1.index_select(-1, x1)
    wy = wy[:, None]
    out = (1 - wy) * ((1 - wx) * a + wx * b) + wy * ((1 - wx) * d + wx * e)
    tapmax = torch.stack([a.abs(), b.abs(), d.abs(), e.abs()]).amax(0)
    return out, tapmax, fy[:, None], fx[None, :]


def resize(x, Hd, Wd):
    """F.interpolate(mode='bilinear', align_corners=False) of pixel-major features x [n, Hs, Ws, C] (values of the storage format) in float64
    -> dict: ref, tapmax [n, Hd, Wd, C]; fy [Hd, 1, 1], fx [Wd, 1]; gy, gx [n, 1, 1, C] = the largest difference of vertically / horizontally neighbouring
    source pixels of the image and channel (errbound.resize_coord_term)"""
    out, tapmax, fy, fx = blend(x.permute(0, 3, 1, 2), Hd, Wd)
    x64 = x.double()
    diff = lambda t: t.abs().amax((1, 2), keepdim=True) if t.numel() else torch.zeros(x.shape[0], 1, 1, x.shape[3], dtype=torch.float64)
    return dict(ref=out.permute(0, 2, 3, 1), tapmax=tapmax.permute(0, 2, 3, 1), fy=fy[..., None], fx=fx[0][:, None],
                gy=diff(x64[:, 1:] - x64[:, :-1]), gx=diff(x64[:, :, 1:] - x64[:, :, :-1]))


def resize_bound(r, out_fmt):
    """the per-element bound of resize_bilinear for resize()'s result"""
    import errbound as EB
    return EB.resize_bound(r['ref'], r['tapmax'], out_fmt, dcoord=EB.resize_coord_term(r['fy'], r['fx'], r['gy'], r['gx']))


RESIZE_SHAPES = ((8, 8, 8, 8), (1, 5, 3, 10), (5, 1, 10, 3), (7, 9, 3, 4), (3, 4, 7, 9), (48, 32, 4, 6), (24, 40, 7, 3), (13, 17, 29, 31))
RESIZE_C = (4, 32, 100)


def resize_case(Hs, Ws, C, fmt, n=2, seed=0):
    """pixel-major features with a steep ramp (one unit per pixel along y, 1.5 along x, centred so that the values near the middle are small against the
    step) plus noise of a third of a step and a per-channel, per-image offset; rounded to the storage format.  A tap that is one pixel off moves the result by
    a whole step, far above the output rounding (2 u |value|, |value| <= 95: at most 0.75 in bf16)."""
    y = torch.arange(Hs, dtype=torch.float32)[:, None, None] - (Hs - 1) / 2
    xx = 1.5 * (torch.arange(Ws, dtype=torch.float32)[None, :, None] - (Ws - 1) / 2)
    off = 0.25 * torch.arange(C, dtype=torch.float32).remainder(5.0)[None, None, :]
    x = torch.stack([(1 + i) * (y + xx) + off for i in range(n)]) + rn(2000 + Hs * 64 + Ws + seed, n, Hs, Ws, C, scale=0.33)
    return x.to(fmt)


# ------------------------------------------------------------------------------------------------------------------------------------------- dino_preprocess
def dino_constants():
    """(mean, std) [3, 1, 1] float64 of the fp32 constants the oracle holds (oracle/dino.py: fp32 tensors)"""
    c = lambda v: torch.from_numpy(np.asarray(v, dtype=F32).astype(np.float64)).view(3, 1, 1)
    return c(IMAGENET_MEAN), c(IMAGENET_STD)


def dino_preprocess(img, Ho, Wo, mean=None, std=None):
    """[-1, 1] -> ImageNet normalise -> bilinear resize (align_corners=False), the reference's order (model/dino.py:61-66): img fp32 [n, 3, H, W] ->
    (ref, max |normalised tap|, per-tap error factor of errbound.dino_tap_err at its largest tap) [n, 3, Ho, Wo], float64"""
    import errbound as EB
    m, s = dino_constants()
    mean = m if mean is None else mean
    std = s if std is None else std
    t = img.double() * 0.5 + 0.5
    nv = (t - mean) / std
    out, tapmax, _, _ = blend(nv, Ho, Wo)
    _, emax, _, _ = blend(EB.dino_tap_err(t, nv, std), Ho, Wo)            # only its max-|tap| output is used
    return out, tapmax, emax


DINO_SHAPES = ((32, 48, 28, 42), (32, 48, 28, 56), (14, 14, 28, 28), (20, 30, 14, 15), (16, 16, 16, 16), (9, 7, 14, 21))


def dino_case(H, W, n=2, seed=0):
    """images in [-1, 1]: a diagonal ramp whose slope differs per channel and image, plus noise"""
    y = torch.linspace(-1, 1, H)[:, None]
    x = torch.linspace(-1, 1, W)[None, :]
    img = torch.stack([torch.stack([(0.5 + 0.1 * c) * y + (0.4 - 0.1 * c + 0.05 * i) * x for c in range(3)]) for i in range(n)])
    return (img + rn(3000 + H * 64 + W + seed, n, 3, H, W, scale=0.1)).clamp(-1, 1).float()


# ------------------------------------------------------------------------------------------------------------------------------------------- exact operations
def mean4(Fm, fmt=None):
    """0.25 (((a + b) + d) + e) in fp32 over the central 2 x 2 pixels (rows 3, 4; columns 3, 4) of every 8 x 8 block of Fm [n, Hm, Wm, C], rounded once to
    the storage format -> [n, Hm / 8, Wm / 8, C]"""
    f = Fm.float()
    a, b, d, e = f[:, 3::8, 3::8], f[:, 3::8, 4::8], f[:, 4::8, 3::8], f[:, 4::8, 4::8]
    return (0.25 * (((a + b) + d) + e)).to(Fm.dtype if fmt is None else fmt)


def add_cast(a, b, b_mod, fmt):
    """rn_fmt(a + b[row % b_mod]) with one fp32 add (b_mod = 0: b[row]; b None: rn_fmt(a))"""
    v = a.float()
    if b is not None:
        rows = torch.arange(a.shape[0])
        v = v + b.float()[rows % b_mod if b_mod > 0 else rows]
    return v.to(fmt)


def patchify(img, p, fmt):
    """img [n, C, H, W] -> rows [n (H/p) (W/p), C p p], column (c p + dy) p + dx, rounded to the storage format"""
    n, C = img.shape[:2]
    return F.unfold(img.float(), kernel_size=p, stride=p).transpose(1, 2).reshape(-1, C * p * p).to(fmt)


def token_embed(ids, tok, pos):
    """tok[ids[b, l]] + pos[l] in fp32 -> [B L, D]; a row whose id is outside [0, vocab) is zero.  -> (rows, status)"""
    B, L = ids.shape
    ok = (ids >= 0) & (ids < tok.shape[0])
    out = tok[ids.long().clamp(0, tok.shape[0] - 1)] + pos[:L][None]
    out = torch.where(ok[..., None], out, torch.zeros_like(out))
    return out.reshape(B * L, -1), (0 if bool(ok.all()) else -1)


def attn_mask(logits):
    """mask[q, k] = logits[q, k] < 0 (1 = blocked; NaN and -0.0 are not below zero: open); a row with every key blocked is cleared"""
    m = logits < 0
    m[m.all(-1)] = False
    return m.to(torch.uint8)


MASK_NK = (1, 100, 255, 256, 257, 700, 4099)
MASK_KINDS = ('random', 'blocked', 'open', 'last', 'second_trip', 'minus_zero', 'specials', 'nan_only', 'blocked_specials')
SUB = float(np.float32(1e-41))           # an fp32 subnormal


def mask_row(kind, Nk, seed):
    """one row of fp32 logits of the given kind"""
    r = rn(4000 + seed, Nk)
    blocked = -r.abs() - 0.1
    if kind == 'random':
        return r
    if kind == 'blocked':
        return blocked
    if kind == 'open':
        return r.abs() + 0.1
    if kind == 'last':                    # blocked everywhere except column Nk - 1
        blocked[Nk - 1] = 0.25
        return blocked
    if kind == 'second_trip':             # blocked everywhere except one column in (255, 511] (the first column where there is none)
        blocked[min(300, Nk - 1) if Nk > 256 else 0] = 0.0
        return blocked
    if kind == 'minus_zero':
        return torch.full((Nk,), -0.0)
    if kind == 'specials':                # NaN, +-inf, +-subnormal among random logits
        for i, v in enumerate((float('nan'), float('inf'), float('-inf'), SUB, -SUB)):
            r[(i * 53 + 1) % Nk] = v
        return r
    if kind == 'nan_only':                # the only key that is not below zero is a NaN: the row stays
        blocked[(Nk - 1) // 2] = float('nan')
        return blocked
    if kind == 'blocked_specials':        # -inf and negative subnormals are below zero: the row is fully blocked and cleared
        blocked[0::3] = float('-inf')
        blocked[1::3] = -SUB
        return blocked
    raise ValueError(kind)


def mask_case(Nk, kinds, seed=0):
    return torch.stack([mask_row(k, Nk, seed + 17 * i + Nk) for i, k in enumerate(kinds)])


ADD_ROWS, ADD_D, ADD_BMOD = 11, (4, 64, 1028), (0, 1, 5, 11)


def add_cast_case(D, fa, fb, seed=0):
    """a [rows, D] and b [rows, D] in their storage formats.  b always has `rows` rows, whatever b_mod: the rows from b_mod on hold other values, so a kernel
    that indexes b by the row itself reads something else but never leaves the buffer"""
    return rn(5000 + D + seed, ADD_ROWS, D).to(fa), rn(5100 + D + seed, ADD_ROWS, D, scale=3.0).to(fb)


TOK_D, TOK_BL, TOK_VOCAB, TOK_NPOS = (8, 256, 768, 1024, 1152), ((1, 1), (3, 7), (5, 64)), 50, 70


def token_case(B, L, D, seed=0):
    """ids int32 [B, L] with 0, vocab - 1 and repeats; tok [vocab, D], pos [npos, D] fp32"""
    g = np.random.Generator(np.random.PCG64(6000 + B * 100 + L + seed))
    ids = torch.from_numpy(g.integers(0, TOK_VOCAB, (B, L)).astype(np.int32))
    flat = ids.view(-1)
    flat[0] = TOK_VOCAB - 1
    if flat.numel() > 2:
        flat[1], flat[-1], flat[-2] = 0, 0, TOK_VOCAB - 1
    return ids, rn(6100 + D, TOK_VOCAB, D), rn(6200 + D, TOK_NPOS, D)
