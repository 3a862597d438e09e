"""SURVEY 8(f) row 2, the input side on the GPU: pst_image_prepare (ImgNorm + antialiased bilinear resize + crop of a decoded uint8 image)
against torch's own antialiased interpolation on the CPU (what torchvision.transforms.Resize applies to a tensor), and pst_patch_rows (the
patch rows of both ViTs in one launch) bit for bit against the separate patchify / DINOv2-preprocess kernels it replaces.

Both are also held to references of their own (tests/input_ref.py; soundness and tightness on the CPU: tests/test_input_host.py): image_prepare to the
float64 triangle filter under errbound.aa_resize_bound at EVERY element, at the shapes where its window rules decide and on images that tell each rule;
patch_rows to the exact patch rows and the float64 DINOv2 preprocessing, between sentinels, at every layout that selects another store path; and the two
wrappers refuse a wrong operand on the host, before anything is launched."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import errbound as EB
import input_ref as IR

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('Hs,Ws,size', [(480, 640, 512), (1200, 1600, 512), (333, 517, 224), (640, 480, 512), (96, 128, 512), (1000, 1000, 512), (540, 960, 512), (500, 700, 384)])
def test_image_prepare_matches_torch_antialias(Hs, Ws, size):
    from panst3r_amd.engine.images import prepare_image, resize_recipe
    g = np.random.Generator(np.random.PCG64(Hs * 7 + Ws))
    img = g.integers(0, 256, size=(Hs, Ws, 3), dtype=np.uint8)
    img[:, :, 1] = (np.arange(Ws)[None, :] * 255 // Ws).astype(np.uint8)          # a ramp: exposes coordinate / transposition mistakes
    out = prepare_image(img, size, 16, DEV)
    (top, left), (Hc, Wc), (Ho, Wo) = resize_recipe(size, 16, Hs, Ws)          # centre crop to the trained aspect ratio, then resize
    assert out.shape == (3, Ho, Wo) and max(Ho, Wo) == size and Ho % 16 == 0 and Wo % 16 == 0
    t = (torch.from_numpy(img).permute(2, 0, 1).float() / 255.0 - 0.5) / 0.5        # ToTensor + Normalize(0.5, 0.5) == ImgNorm
    ref = F.interpolate(t[None][:, :, top:top + Hc, left:left + Wc], size=(Ho, Wo), mode='bilinear', align_corners=False, antialias=True)[0]
    assert float((out.cpu() - ref).abs().max()) < 2e-5
    assert float(out.min()) >= -1.0001 and float(out.max()) <= 1.0001
    crop = torch.from_numpy(img[top:top + Hc, left:left + Wc])                       # every element against the float64 filter, under its own bound
    EB.check(out, IR.aa_resize(crop, Ho, Wo, 0, 0, Ho, Wo)[0], EB.aa_resize_bound(IR.img_norm(crop), (Ho, Wo), (0, 0, Ho, Wo)), 'image_prepare %dx%d' % (Hs, Ws))


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('H,W', [(64, 96), (384, 512), (96, 64)])
def test_patch_rows_bit_identical_to_separate_kernels(dtype, H, W):
    from panst3r_amd import hip
    n = 3
    g = np.random.Generator(np.random.PCG64(H + W))
    img = torch.from_numpy(g.uniform(-1, 1, size=(n, 3, H, W)).astype(np.float32)).to(DEV)
    T = (H // 16) * (W // 16)
    enc = torch.full((n * T, 768), 7.0, dtype=dtype, device=DEV)
    dino = torch.full((n * T, 640), 7.0, dtype=dtype, device=DEV)
    hip.patch_rows(img, enc=enc, dino=dino, p_enc=16, p_dino=14)
    ref_e = torch.full((n * T, 768), 7.0, dtype=dtype, device=DEV)
    hip.patchify(img, ref_e, 16)
    pre = torch.empty(n, 3, H // 16 * 14, W // 16 * 14, device=DEV)
    hip.dino_preprocess(img, pre)
    ref_d = torch.full((n * T, 640), 7.0, dtype=dtype, device=DEV)
    hip.patchify(pre, ref_d, 14)
    assert torch.equal(enc, ref_e) and torch.equal(dino, ref_d)
    # either output alone
    e2 = torch.empty_like(enc); hip.patch_rows(img, enc=e2, p_enc=16)
    d2 = torch.empty_like(dino); hip.patch_rows(img, dino=d2, p_enc=16, p_dino=14)
    assert torch.equal(e2, ref_e) and torch.equal(d2, ref_d)
    # DINOv2 on the transposed image (portrait views) without a transposed copy
    imt = img.transpose(2, 3).contiguous()
    pre_t = torch.empty(n, 3, W // 16 * 14, H // 16 * 14, device=DEV)
    hip.dino_preprocess(imt, pre_t)
    ref_t = torch.empty_like(dino); hip.patchify(pre_t, ref_t, 14)
    d3 = torch.empty_like(dino); hip.patch_rows(img, dino=d3, p_enc=16, p_dino=14, dino_transposed=True)
    assert torch.equal(d3, ref_t)


def test_load_images_pair_and_shapes(tmp_path):
    """reference load_images contract (tools/demo_panst3r.py:94-114): dict(img, true_shape), long side = size, a lone image is duplicated."""
    import PIL.Image
    from panst3r_amd.engine.images import load_images
    g = np.random.Generator(np.random.PCG64(3))
    arr = g.integers(0, 256, size=(300, 400, 3), dtype=np.uint8)
    path = tmp_path / 'a.png'
    PIL.Image.fromarray(arr).save(path)
    views = load_images([str(path)], size=512, patch_size=16, verbose=False, device=DEV)
    assert len(views) == 2 and views[0]['img'].shape == (3, 384, 512) and list(views[0]['true_shape']) == [384, 512]
    again = load_images([arr, arr[:, ::-1].copy()], size=224, verbose=False, device=DEV)
    assert again[0]['img'].shape == (3, 224, 224)              # 224 is a trained resolution: centre crop to 1:1, then resize
    assert float((again[0]['img'].flip(-1) - again[1]['img']).abs().max()) < 1e-4          # the filter is symmetric: mirrored input, mirrored output


@pytest.mark.parametrize('case', list(IR.IMAGE_CASES))
def test_image_prepare_cases(case):
    """every image kind at the case: the conditions the case was built for hold on the reference; the identity resize is ImgNorm in fp32 bit for bit, every
    other output is under its bound; nothing is written behind the output"""
    from panst3r_amd import hip
    Hs, Ws, Hr, Wr, top, left, H, W = IR.IMAGE_CASES[case]
    worst = 0.0
    for kind in IR.IMAGE_KINDS:
        img = IR.image(kind, case)
        ref = IR.aa_resize(img, Hr, Wr, top, left, H, W)[0]
        IR.image_conditions(case, kind, ref)
        out = torch.full((3 * H * W + 64,), float('nan'), device=DEV)
        hip.image_prepare(img.to(DEV), out[:3 * H * W].view(3, H, W), (Hr, Wr), (top, left))
        got = out.cpu()
        assert bool(torch.isnan(got[3 * H * W:]).all()), kind
        got = got[:3 * H * W].view(3, H, W)
        if case == 'identity':
            assert torch.equal(got, (img.permute(2, 0, 1).float() / 255.0 - 0.5) / 0.5), kind
        worst = max(worst, EB.check(got, ref, EB.aa_resize_bound(IR.img_norm(img), (Hr, Wr), (top, left, H, W)), 'image_prepare %s %s' % (case, kind)))
    print('image_prepare %s: largest |err| / bound %.3f' % (case, worst))


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16], ids=['f16', 'bf16'])
@pytest.mark.parametrize('layout', list(IR.PATCH_LAYOUTS))
def test_patch_rows_layouts(layout, dtype):
    """both outputs between sentinels at a layout that selects one store path of each half (input_ref.PATCH_LAYOUTS), landscape, portrait and portrait with
    the transposed DINOv2 input: the encoder half exact, the DINOv2 half under its bound, the padding zero, every sentinel intact; a second call writes the
    same bytes"""
    from panst3r_amd import hip
    worst = 0.0
    for H, W, transposed in IR.PATCH_SHAPES:
        T = (H // IR.P_ENC) * (W // IR.P_ENC)
        img = IR.patch_image(H, W, layout, DEV)
        enc_ref, dino_ref, dino_bound = IR.patch_refs(img, transposed, dtype)
        stores = []
        for _ in range(2):
            bufs = IR.patch_buffers(layout, T, dtype, DEV)
            IR.patch_branches(layout, bufs['enc'][1].data_ptr(), img.data_ptr(), bufs['dino'][1].data_ptr())
            hip.patch_rows(img, enc=bufs['enc'][1], dino=bufs['dino'][1], p_enc=IR.P_ENC, p_dino=IR.P_DINO, dino_transposed=transposed)
            worst = max(worst, IR.check_patch_buffers(bufs, enc_ref, dino_ref, dino_bound, 'patch_rows %s %dx%d%s' % (layout, H, W, ' transposed' if transposed else '')))
            stores.append(bufs)
        assert torch.equal(stores[0]['enc'][0], stores[1]['enc'][0]) and torch.equal(stores[0]['dino'][0], stores[1]['dino'][0])
    print('patch_rows %s: largest DINOv2 |err| / bound %.3f' % (layout, worst))


@pytest.fixture
def recorder(monkeypatch):
    """hip._call replaced by a recorder (tests/test_hip_operand_refusals.py): NOTHING RUNS ON THE DEVICE, a bad operand can only be refused on the host"""
    from panst3r_amd import hip
    rec = []
    monkeypatch.setattr(hip, '_call', lambda what, *args: rec.append((what, args)))
    return rec


def refused(recorder, what, call, kept):
    del recorder[:]
    with pytest.raises(RuntimeError, match='^%s: ' % what):
        call()
    assert not recorder, 'a launch was made'
    assert all(bool((t == IR.SENTINEL).all()) for t in kept)


def test_patch_rows_refuses_wrong_operands_before_any_launch(recorder):
    from panst3r_amd import hip
    n, H, W, rows = 2, 32, 48, 12
    z = lambda *shape, dtype=torch.bfloat16: torch.full(shape, IR.SENTINEL, dtype=dtype, device=DEV)
    img, enc, dino = z(n, 3, H, W, dtype=torch.float32), z(rows, 768), z(rows, 640)
    hip.patch_rows(img, enc=enc, dino=dino)
    assert len(recorder) == 1 and recorder[0][0] == 'pst_patch_rows'
    sent = recorder[0][1]
    assert sent[:5] == (img.data_ptr(), enc.data_ptr(), 768, dino.data_ptr(), 640) and sent[5:] == (n, H, W, 16, 14, False, 0)
    bad = {
        'enc one row short': dict(enc=z(rows - 1, 768)),
        'dino one row short': dict(dino=z(rows - 1, 640)),
        'enc one column short': dict(enc=z(rows, 767)),
        'dino one column short': dict(dino=z(rows, 587)),
        'enc not 2-D': dict(enc=z(rows, 768, 1)),
        'enc column-major': dict(enc=z(768, rows).t()),
        'rows that overlap': dict(enc=z(rows * 768).as_strided((rows, 768), (700, 1))),
        'padding of the last row beyond the storage': dict(enc=z((rows - 1) * 1024 + 768).as_strided((rows, 768), (1024, 1))),
        'two 16-bit formats': dict(dino=z(rows, 640, dtype=torch.float16)),
        '16 bit and fp32': dict(dino=z(rows, 640, dtype=torch.float32)),
        'an integer output': dict(enc=z(rows, 768, dtype=torch.int16), dino=None),
        'enc on the CPU': dict(enc=z(rows, 768).cpu()),
        'img on the CPU': dict(img=img.cpu()),
        'img in 16 bit': dict(img=z(n, 3, H, W)),
        'img strided': dict(img=z(n, 3, H, 2 * W, dtype=torch.float32)[..., ::2]),
        'four channels': dict(img=z(n, 4, H, W, dtype=torch.float32)),
        'H no multiple of p_enc': dict(img=z(n, 3, 40, W, dtype=torch.float32)),
        'p_enc = 0': dict(p_enc=0),
        'neither output': dict(enc=None, dino=None),
    }
    for name, change in bad.items():
        kw = dict(dict(img=img, enc=enc, dino=dino), **change)
        refused(recorder, 'patch_rows', lambda: hip.patch_rows(kw.pop('img'), **kw), [t for t in (enc, dino) if t is not None])
    # what the production callers pass goes through: either output alone, fp32 outputs, a wider leading dimension, more rows than needed
    del recorder[:]
    hip.patch_rows(img, enc=enc)
    hip.patch_rows(img, dino=dino, dino_transposed=True)
    hip.patch_rows(img, enc=z(rows, 768, dtype=torch.float32), dino=z(rows, 640, dtype=torch.float32))
    hip.patch_rows(img, enc=z(rows + 3, 1024)[:, :776], dino=z(rows, 588))
    assert [r[1][2] for r in recorder] == [768, 0, 768, 1024] and len(recorder) == 4


def test_image_prepare_refuses_wrong_operands_before_any_launch(recorder):
    from panst3r_amd import hip
    Hs, Ws, H, W = 20, 30, 16, 16
    src = torch.zeros(Hs, Ws, 3, dtype=torch.uint8, device=DEV)
    out = torch.full((3, H, W), IR.SENTINEL, device=DEV)
    hip.image_prepare(src, out, (18, 24), (2, 8))
    assert recorder == [('pst_image_prepare', (src.data_ptr(), Hs, Ws, out.data_ptr(), 18, 24, 2, 8, H, W))]
    bad = {
        'the crop ends one row behind the resized image': dict(crop_origin=(3, 8)),
        'the crop ends one column behind the resized image': dict(crop_origin=(2, 9)),
        'a negative origin': dict(crop_origin=(-1, 0)),
        'a resized height of 0': dict(resized=(0, 24), crop_origin=(0, 0)),
        'out with four channels': dict(out=torch.full((4, H, W), IR.SENTINEL, device=DEV)),
        'out not contiguous': dict(out=torch.full((3, H, 2 * W), IR.SENTINEL, device=DEV)[..., ::2]),
        'out in 16 bit': dict(out=out.half()),
        'an empty out': dict(out=torch.full((3, 0, W), IR.SENTINEL, device=DEV)),
        'src with four channels': dict(src_u8=torch.zeros(Hs, Ws, 4, dtype=torch.uint8, device=DEV)),
        'src planar': dict(src_u8=torch.zeros(3, Hs, Ws, dtype=torch.uint8, device=DEV).permute(1, 2, 0)),
        'src in int32': dict(src_u8=src.int()),
        'src on the CPU': dict(src_u8=src.cpu()),
        'out on the CPU': dict(out=out.cpu()),
    }
    for name, change in bad.items():
        kw = dict(dict(src_u8=src, out=out, resized=(18, 24), crop_origin=(2, 8)), **change)
        refused(recorder, 'image_prepare', lambda: hip.image_prepare(**kw), [out])
