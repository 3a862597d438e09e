"""Float64 / exact restatements of the two image input kernels of csrc/image.hip, written from the header's description (include/panst3r_hip.h) and not
from the kernels, with the cases at which their window, alignment and padding rules decide.  Nothing here imports the code under test.

image_prepare: `aa_resize` is ImgNorm, the antialiased bilinear (triangle) filter per axis and the crop, in float64 with the tap weights from exact integer
arithmetic; held under errbound.aa_resize_bound.  patch_rows: the encoder half is smallops_ref.patchify (exact), the DINOv2 half
smallops_ref.dino_preprocess (float64) rearranged into patch rows, held under errbound.resize_bound; `patch_buffers` / `check_patch_buffers` allocate and
check the outputs between sentinels at every layout that selects another store path of the kernel.

tests/test_input_host.py proves on the CPU that an fp32 emulation of each kernel meets these checks and that the planted mistakes fail them;
tests/test_hip_input.py holds the kernels to the same references at the same cases.
"""
import numpy as np
import torch
import torch.nn.functional as F

import smallops_ref as SR


# ------------------------------------------------------------------------------------------------------------------------------------------- image_prepare
def aa_weights(n_in, n_out):
    """[n_out, n_in] float64: row i = the triangle of half-width s = max(n_in / n_out, 1) around (i + 0.5) n_in / n_out, sampled at the pixel centres j + 0.5
    of ALL source pixels and normalised to sum 1.  (j + 0.5 - c) / s = ((2 j + 1) n_out - (2 i + 1) n_in) / (2 max(n_in, n_out)): numerator and the weight
    sums are exact integers, one float64 division per weight."""
    i = torch.arange(n_out, dtype=torch.int64)[:, None]
    j = torch.arange(n_in, dtype=torch.int64)[None, :]
    den = 2 * max(n_in, n_out)
    t = (den - ((2 * j + 1) * n_out - (2 * i + 1) * n_in).abs()).clamp_min(0)
    return t.double() / t.sum(1, keepdim=True).double()


def img_norm(img_u8):
    """ImgNorm = ToTensor + Normalize(0.5, 0.5) in float64: uint8 [Hs, Ws, 3] -> [3, Hs, Ws] in [-1, 1]"""
    return (torch.as_tensor(img_u8).permute(2, 0, 1).double() / 255.0 - 0.5) / 0.5


def aa_resize(img_u8, Hr, Wr, top, left, H, W):
    """uint8 [Hs, Ws, 3] -> (ref float64 [3, H, W], Wy [H, Hs], Wx [W, Ws]): ImgNorm, the antialiased resize to (Hr, Wr), the crop
    [top, top + H) x [left, left + W).  The filter is separable: the weight rows of the kept outputs are returned too."""
    p = img_norm(img_u8)
    Wy = aa_weights(p.shape[1], Hr)[top:top + H]
    Wx = aa_weights(p.shape[2], Wr)[left:left + W]
    return torch.matmul(torch.matmul(Wy, p), Wx.T), Wy, Wx


# (Hs, Ws, Hr, Wr, top, left, H, W): the smallest shapes at which each window rule decides
IMAGE_CASES = {
    'identity': (16, 24, 16, 24, 0, 0, 16, 24),                   # must reproduce ImgNorm bit for bit; the second tap of every window weighs exactly 0
    '2to1': (32, 48, 16, 24, 0, 0, 16, 24),                       # dyadic weights, no coordinate error
    '4to1': (64, 96, 16, 24, 0, 0, 16, 24),
    '3to2': (24, 36, 16, 24, 0, 0, 16, 24),                       # the scale is exact in fp32, the weights are not dyadic
    'upscale': (13, 29, 32, 48, 0, 0, 32, 48),                    # inexact scale, support clamped to 1
    'crop_inside': (37, 53, 20, 31, 3, 5, 16, 24),                # inexact scale, crop in the interior
    'crop_to_the_end': (37, 53, 20, 31, 4, 7, 16, 24),            # the crop ends on the last resized row and column
    'one_source_row': (1, 40, 16, 16, 0, 0, 16, 16),
    'tall_window': (200, 7, 5, 32, 1, 0, 4, 32),                  # 40:1 in y (about 80 taps), up-scaling in x, four output rows
    'below_one_wave': (40, 40, 7, 9, 0, 0, 7, 9),                 # 63 output pixels
    'one_output': (40, 40, 1, 1, 0, 0, 1, 1),
    # the shapes of test_image_prepare_matches_torch_antialias after the centre crop of engine.images.resize_recipe (tests/test_input_host.py checks that)
    '480x640': (480, 640, 384, 512, 0, 0, 384, 512),
    '1200x1600': (1200, 1600, 384, 512, 0, 0, 384, 512),
    '333x517': (333, 333, 224, 224, 0, 0, 224, 224),
    '640x480': (640, 480, 512, 384, 0, 0, 512, 384),
    '96x128': (96, 128, 384, 512, 0, 0, 384, 512),
    '1000x1000': (750, 1000, 384, 512, 0, 0, 384, 512),
    '540x960': (540, 960, 288, 512, 0, 0, 288, 512),
    '500x700': (496, 700, 272, 384, 0, 0, 272, 384),
}
RECIPE_CASES = {'480x640': (480, 640, 512), '1200x1600': (1200, 1600, 512), '333x517': (333, 517, 224), '640x480': (640, 480, 512), '96x128': (96, 128, 512),
                '1000x1000': (1000, 1000, 512), '540x960': (540, 960, 512), '500x700': (500, 700, 384)}
SMALL_CASES = tuple(k for k in IMAGE_CASES if k not in RECIPE_CASES)
IMAGE_KINDS = ('noise', 'zero', 'grey', 'white', 'impulse', 'ramp', 'planes')


def _nonzero_taps(n_in, n_out):
    """the largest number of source pixels with a non-zero weight in one output's window"""
    return int((aa_weights(n_in, n_out) > 0).sum(1).max())


def impulse_rows(n_in, n_out):
    """positions of the impulses along one axis: a comb whose period is one more than the widest window, so that no window holds two of them and every output
    shows the weight of ONE tap; the phase puts an impulse half a period in (the only one of a short axis)"""
    period = _nonzero_taps(n_in, n_out) + 1
    return list(range(min(period // 2, n_in - 1), n_in, period))


def image(kind, case, seed=0):
    """uint8 [Hs, Ws, 3] of the given kind (seeded by the case's shape):
      noise   - every tap matters, nothing cancels by symmetry;
      zero, grey, white - constant 0 / 128 / 255: the weights are a partition of unity, so the output is the constant - a wrong normalisation is not;
      impulse - 255 on 0 at a comb of isolated pixels (impulse_rows): the output is -1 + 2 wy wx of the ONE tap in the window, every weight on its own;
      ramp    - 97 grey levels down the rows, 151 along the columns: a transposition, a half-pixel offset or an exchanged scale moves every output;
      planes  - a column ramp, a row ramp and noise in the three channels: channel order and HWC -> CHW."""
    Hs, Ws, Hr, Wr = IMAGE_CASES[case][:4]
    g = np.random.Generator(np.random.PCG64(Hs * 7 + Ws + 1000 * seed))
    y, x = np.arange(Hs)[:, None], np.arange(Ws)[None, :]
    img = np.zeros((Hs, Ws, 3), dtype=np.int64)
    if kind == 'noise':
        img = g.integers(0, 256, size=(Hs, Ws, 3))
    elif kind in ('zero', 'grey', 'white'):
        img[:] = {'zero': 0, 'grey': 128, 'white': 255}[kind]
    elif kind == 'impulse':
        img[np.ix_(impulse_rows(Hs, Hr), impulse_rows(Ws, Wr))] = 255
    elif kind == 'ramp':
        img[:] = (y * 97 // Hs + x * 151 // Ws)[:, :, None] + 3 * np.arange(3)[None, None, :]
    elif kind == 'planes':
        img[:, :, 0] = x * 255 // Ws
        img[:, :, 1] = 255 - y * 255 // Hs
        img[:, :, 2] = g.integers(0, 256, size=(Hs, Ws))
    else:
        raise ValueError(kind)
    assert img.min() >= 0 and img.max() <= 255
    return torch.from_numpy(img.astype(np.uint8))


def fp32_exact_scale(n_in, n_out):
    """True when n_in / n_out and every centre (i + 0.5) n_in / n_out are fp32 numbers"""
    s = np.float32(n_in) / np.float32(n_out)
    c = (np.arange(n_out, dtype=np.float64) + 0.5) * float(s)
    return float(s) * n_out == n_in and bool((c.astype(np.float32).astype(np.float64) == c).all())


# what each case was built for, asserted on the reference: (clipped at the low border, clipped at the high border) per axis (y, x), the tap count of the
# widest window per axis, fp32-exact scale per axis.  A window is clipped when a pixel centre beyond the image (-0.5 or n_in + 0.5) would carry weight: the kept taps no longer sum to s.
IMAGE_EXPECT = {
    'identity': dict(low=(False, False), high=(False, False), taps=(1, 1), exact=(True, True)),
    '2to1': dict(low=(True, True), high=(True, True), taps=(4, 4), exact=(True, True)),
    '4to1': dict(low=(True, True), high=(True, True), taps=(8, 8), exact=(True, True)),
    '3to2': dict(low=(True, True), high=(True, True), taps=(3, 3), exact=(True, True)),
    'upscale': dict(low=(True, True), high=(True, True), taps=(2, 2), exact=(True, False)),                 # 13 / 32 is dyadic, 29 / 48 is not
    'crop_inside': dict(low=(False, False), high=(False, False), taps=(4, 4), exact=(False, False)),
    'crop_to_the_end': dict(low=(False, False), high=(True, True), taps=(4, 4), exact=(False, False)),
    'one_source_row': dict(low=(True, True), high=(True, True), taps=(1, 5), exact=(True, True)),
    'tall_window': dict(low=(False, True), high=(True, True), taps=(80, 2), exact=(True, True)),
    'below_one_wave': dict(low=(True, True), high=(True, True), taps=(12, 9), exact=(False, False)),
    'one_output': dict(low=(True, True), high=(True, True), taps=(40, 40), exact=(True, True)),
}


def image_conditions(case, kind=None, ref=None):
    """assert on the reference what the case was built for (IMAGE_EXPECT; the recipe shapes carry none), and for the impulse image that no window holds two
    impulses and that at least a quarter of the outputs show one"""
    Hs, Ws, Hr, Wr, top, left, H, W = IMAGE_CASES[case]
    assert Hs > 0 and Ws > 0 and 0 <= top and top + H <= Hr and 0 <= left and left + W <= Wr and H > 0 and W > 0
    exp = IMAGE_EXPECT.get(case)
    for ax, (n_in, n_out, lo, n) in enumerate(((Hs, Hr, top, H), (Ws, Wr, left, W))):
        s = max(n_in / n_out, 1.0)
        c = (np.arange(lo, lo + n) + 0.5) * n_in / n_out
        taps = (aa_weights(n_in, n_out)[lo:lo + n] > 0).sum(1)
        if exp is not None:
            assert bool((c - s < -0.5).any()) == exp['low'][ax], (case, ax, 'low')
            assert bool((c + s > n_in + 0.5).any()) == exp['high'][ax], (case, ax, 'high')
            assert int(taps.max()) == exp['taps'][ax], (case, ax, int(taps.max()))
            assert fp32_exact_scale(n_in, n_out) == exp['exact'][ax], (case, ax, 'exact')
    if kind == 'impulse':
        for n_in, n_out in ((Hs, Hr), (Ws, Wr)):
            hit = (aa_weights(n_in, n_out)[:, impulse_rows(n_in, n_out)] > 0).sum(1)
            assert int(hit.max()) <= 1
        assert ref is not None and float((ref[0] != -1.0).double().mean()) >= 0.25, (case, float((ref[0] != -1.0).double().mean()))


# ------------------------------------------------------------------------------------------------------------------------------------------- patch_rows
P_ENC, P_DINO, K_ENC, K_DINO = 16, 14, 3 * 16 * 16, 3 * 14 * 14
PATCH_N = 2
PATCH_SHAPES = ((32, 48, False), (48, 32, False), (48, 32, True))          # (H, W, dino_transposed): T = 6, 2 * 6 * 92 = 1104 threads, no multiple of 256
# layout -> leading dimensions and the element offsets of the operands inside their allocations.  The first comment of each line is the branch of
# patch_rows_kernel it selects, derived from the alignment tests of the source (image.hip): the encoder's vector path needs ld_enc % 8 == 0 and 16-byte
# aligned enc and img; the DINOv2 pair stores need an even ld_dino and a 4-byte aligned dino.
PATCH_LAYOUTS = {
    'baseline': dict(ld_enc=768, ld_dino=640),                              # vector paths (every earlier test)
    'padded_enc': dict(ld_enc=776, ld_dino=588),                            # vector paths; zero padding on enc only, none on dino
    'ld_enc_772': dict(ld_enc=772, ld_dino=640),                            # ld_enc & 7: scalar encoder path
    'enc_offset': dict(ld_enc=768, ld_dino=640, enc_off=1),                 # enc 2 bytes off a 16-byte boundary: scalar encoder path
    'img_offset': dict(ld_enc=768, ld_dino=640, img_off=1),                 # img 4 bytes off a 16-byte boundary: scalar encoder path
    'ld_dino_589': dict(ld_enc=768, ld_dino=589),                           # odd ld_dino: single stores
    'dino_offset': dict(ld_enc=768, ld_dino=640, dino_off=1),               # dino 2 bytes off a 4-byte boundary: single stores
}
SENTINEL = 7.0
GUARD_ROWS, GUARD_TAIL = 2, 64


def patch_branches(layout, enc_ptr, img_ptr, dino_ptr):
    """(encoder vector path, DINOv2 pair stores) for the operands' addresses, by the rule above; asserts that the layout selects what its line says"""
    L = PATCH_LAYOUTS[layout]
    vec = L['ld_enc'] % 8 == 0 and enc_ptr % 16 == 0 and img_ptr % 16 == 0
    pairs = L['ld_dino'] % 2 == 0 and dino_ptr % 4 == 0
    assert vec == (layout in ('baseline', 'padded_enc', 'ld_dino_589', 'dino_offset')), (layout, enc_ptr % 16, img_ptr % 16)
    assert pairs == (layout not in ('ld_dino_589', 'dino_offset')), (layout, dino_ptr % 4)
    return vec, pairs


def patch_image(H, W, layout, device='cpu'):
    """fp32 images [PATCH_N, 3, H, W] in [-1, 1] (smallops_ref.dino_case: per-channel, per-image ramps plus noise), a contiguous view `img_off` floats into
    their allocation"""
    off = PATCH_LAYOUTS[layout].get('img_off', 0)
    img = SR.dino_case(H, W, n=PATCH_N, seed=H)
    store = torch.zeros(off + img.numel() + 4, dtype=torch.float32, device=device)
    view = store[off:off + img.numel()].view(img.shape)
    view.copy_(img)
    return view


def patch_buffers(layout, T, fmt, device='cpu'):
    """-> {'enc': (allocation, view [PATCH_N T, ld_enc]), 'dino': ...}: every allocation is SENTINEL throughout and holds, behind the operand's offset,
    GUARD_ROWS rows, the operand's rows, GUARD_ROWS rows and a tail of GUARD_TAIL elements"""
    L = PATCH_LAYOUTS[layout]
    out = {}
    for name in ('enc', 'dino'):
        ld, off, rows = L['ld_' + name], L.get(name + '_off', 0), PATCH_N * T
        store = torch.full((off + (rows + 2 * GUARD_ROWS) * ld + GUARD_TAIL,), SENTINEL, dtype=fmt, device=device)
        first = off + GUARD_ROWS * ld
        out[name] = (store, store[first:first + rows * ld].view(rows, ld))
    return out


def patch_refs(img, transposed, fmt):
    """-> (encoder rows in fmt, exact; DINOv2 rows float64 [n T, K_DINO]; their bound): the header's two halves from the references of the sibling kernels"""
    import errbound as EB
    img = img.detach().cpu().contiguous()
    n, _, H, W = img.shape
    enc = SR.patchify(img, P_ENC, fmt)
    src = img.transpose(2, 3).contiguous() if transposed else img
    Ho, Wo = src.shape[2] // P_ENC * P_DINO, src.shape[3] // P_ENC * P_DINO
    rows = lambda t: F.unfold(t, kernel_size=P_DINO, stride=P_DINO).transpose(1, 2).reshape(-1, K_DINO)
    ref, tapmax, emax = SR.dino_preprocess(src, Ho, Wo)
    return enc, rows(ref), EB.resize_bound(rows(ref), rows(tapmax), fmt, dtaps=rows(emax))


def check_patch_buffers(bufs, enc_ref, dino_ref, dino_bound, what):
    """the two outputs against their references, and the memory around them: columns K .. ld - 1 of every row zero, every sentinel untouched (the offset
    elements, the guard rows before and after - so nothing behind row n T - 1 is written - and the tail).  Returns the DINOv2 half's largest err / bound."""
    import errbound as EB
    ratio = 0.0
    for name, K, ref in (('enc', K_ENC, enc_ref), ('dino', K_DINO, dino_ref)):
        store, view = bufs[name]
        store, rows, ld = store.detach().cpu(), view.shape[0], view.shape[1]
        first = view.data_ptr() - bufs[name][0].data_ptr()
        assert first % store.element_size() == 0
        first //= store.element_size()
        got = store[first:first + rows * ld].view(rows, ld)
        before, after = store[:first], store[first + rows * ld:]
        assert before.numel() >= GUARD_ROWS * ld and after.numel() == GUARD_ROWS * ld + GUARD_TAIL
        assert bool((before == SENTINEL).all()), '%s: %s: %d elements before the first row were written' % (what, name, int((before != SENTINEL).sum()))
        assert bool((after == SENTINEL).all()), '%s: %s: %d elements behind the last row were written, the first %d behind it' % (
            what, name, int((after != SENTINEL).sum()), int((after != SENTINEL).nonzero()[0]))
        pad = got[:, K:]
        assert bool((pad == 0).all()), '%s: %s: %d of the padding columns %d .. %d are not zero' % (what, name, int((pad != 0).sum()), K, ld - 1)
        if name == 'enc':
            bad = got[:, :K] != ref
            assert not bool(bad.any()), '%s: enc: %d elements differ from the rounded image, the first at %s' % (what, int(bad.sum()), bad.nonzero()[0].tolist())
        else:
            ratio = EB.check(got[:, :K], ref, dino_bound, what + ': dino')
    return ratio
