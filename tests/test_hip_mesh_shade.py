"""csrc/mesh_normals.hip and pst_mesh_interp of csrc/mesh.hip against tests/mesh_shade_ref.py on the GPU, bit for bit: the vertex normals at the
workgroup edges, on one vertex shared by 4 096 faces, with bad faces and at odd extents; the interpolation and the shade over rendered face maps of
the mesh tests' scene and over hand-made maps (entries that are no face, faces that are not drawn or do not cover their pixel, the corner exchange,
the launch edges); the refusals; `PanopticMesh.render_color` and the PLY file with normals end to end.  Every output sits inside a canary-padded
allocation and every launch runs twice with equal bytes."""
import functools

import numpy as np
import pytest
import torch

import mesh_ref as M
import mesh_shade_ref as S
from panst3r_amd import hip
from panst3r_amd.engine import render_mesh, mesh_camera_table, vertex_normals, interpolate_render, shade_render, load_ply_mesh

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F = np.float32
PAD = 256                                                                      # canary bytes on either side of an output
CANARY = 0xA5


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


class Padded:
    """a tensor of `shape` in the middle of a byte buffer whose PAD bytes on either side hold the canary; the tensor itself starts as canaries too"""

    def __init__(self, shape, dtype):
        n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        self.buf = torch.full((PAD + n + PAD,), CANARY, dtype=torch.uint8, device=DEV)
        self.t = self.buf[PAD:PAD + n].view(dtype).view(*shape)
        self.n = n

    def intact(self):
        return bool((self.buf[:PAD] == CANARY).all()) and bool((self.buf[PAD + self.n:] == CANARY).all())

    def untouched(self):
        return bool((self.buf == CANARY).all())


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def faces32(faces, Nv):
    """the indices AS THEY ARE, as int32: -1, Nv and 2^31 - 1 reach the kernels, whose own test of every index is what keeps them inside the vertices"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    assert (f >= -2 ** 31).all() and (f < 2 ** 31).all()
    return f.astype(np.int32)


# ---------------------------------------------------------------- vertex normals
def run_normals(v, f):
    """hip.mesh_normals twice into padded buffers -> float32 [Nv, 3]"""
    v = np.asarray(v, dtype=F).reshape(-1, 3)
    Nv = len(v)
    vd, fd = dev(v), dev(faces32(f, Nv))
    outs = []
    for _ in range(2):
        acc, out = Padded((Nv, 3, 2), torch.int64), Padded((Nv, 3), torch.float32)
        hip.mesh_normals(vd, fd, S.shift(v), acc.t, out.t)
        torch.cuda.synchronize()
        assert acc.intact() and out.intact()
        assert np.array_equal(acc.t.cpu().numpy(), S.accumulate(v, f))
        outs.append(out.t.cpu().numpy())
    assert np.array_equal(bits(outs[0]), bits(outs[1]))
    return outs[0]


def check_normals(v, f):
    v = np.asarray(v, dtype=F).reshape(-1, 3)
    got, want = run_normals(v, f), S.normals(v, f)
    assert got.dtype == want.dtype and np.array_equal(bits(got), bits(want)), int((bits(got) != bits(want)).sum())
    eng = vertex_normals(dev(v), dev(np.asarray(f, dtype=np.int64).reshape(-1, 3)))         # the public entry point: its own extent; int64 faces, bad ones made -1
    assert np.array_equal(bits(eng), bits(want))
    return want


def random_mesh(seed, Nv, Nf, scale=1.0):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, (Nv, 3)) * scale).astype(F), rng.integers(0, Nv, (Nf, 3))


@pytest.mark.parametrize('Nf', [1, 255, 256, 257])
def test_normals_at_the_workgroup_edges(Nf):
    v, f = random_mesh(Nf, 100, Nf)
    f[0] = [0, 1, 2]
    n = check_normals(v, f)
    assert n[:3].any(axis=1).all()


@functools.lru_cache(maxsize=None)
def fan():
    """vertex 0 at the centre of 4 096 thin faces to a jittered rim: mixed-sign face vectors, every one of them added to the same 6 words"""
    rng = np.random.default_rng(21)
    n = 4096
    a = np.sort(rng.uniform(0, 2 * np.pi, n + 1))
    rim = np.stack([np.cos(a) * rng.uniform(0.5, 1, n + 1), np.sin(a) * rng.uniform(0.5, 1, n + 1), rng.uniform(-0.5, 0.5, n + 1)], axis=1)
    v = np.concatenate([[[0.03, -0.02, 0.01]], rim]).astype(F)
    f = np.stack([np.zeros(n, dtype=np.int64), np.arange(1, n + 1), np.arange(2, n + 2)], axis=1)
    f[::3] = f[::3, ::-1]                                                      # every third face wound the other way
    return v, f


def test_one_vertex_shared_by_4096_faces_and_the_order_of_the_faces():
    v, f = fan()
    acc = S.accumulate(v, f)
    valid, idx = S.valid_faces(v, f)
    q = np.rint(np.ldexp(S.face_vectors(v, idx), S.shift(v))).astype(np.int64)
    assert valid.all() and (q < 0).any(axis=0).all() and (q > 0).any(axis=0).all()           # both signs on every axis: the floor split is exercised
    assert (acc[0, :, 1] > (500 << 26)).all()                                                # the lo words carried past 2^26 hundreds of times
    want = check_normals(v, f)
    assert want[0].any()
    perm = np.random.default_rng(22).permutation(len(f))
    for order in (f[::-1], f[perm]):
        got = run_normals(v, order)
        assert np.array_equal(bits(got), bits(want))


def test_bad_faces_an_isolated_vertex_and_a_mesh_of_one_vertex():
    v, f = random_mesh(31, 40, 60)
    v[7] = [np.nan, 0.5, 0.5]
    f = f[(f != 39).all(axis=1) & (f != 7).all(axis=1)]                        # vertex 39 is on no face
    bad = np.array([[0, -1, 2], [0, 1, len(v)], [3, 7, 4], [5, 5, 6], [2 ** 31 - 1, 0, 1], [len(v), len(v), len(v)], [1, 2, -2 ** 31]])
    f = np.concatenate([bad[:2], f[:20], bad[2:4], f[20:], bad[4:]])
    assert sorted(set(faces32(f, len(v)).ravel()) - set(range(len(v)))) == [-2 ** 31, -1, len(v), 2 ** 31 - 1]      # what the accumulate kernel is given
    n = check_normals(v, f)
    assert not n[39].any() and not n[7].any() and n[0].any()
    assert np.array_equal(bits(n), bits(S.normals(v, [r for r in f.tolist() if r not in bad.tolist()])))     # the bad faces add nothing
    one = check_normals(np.array([[1.5, -2.0, 0.25]], dtype=F), np.array([[0, 0, 0]]))
    assert one.shape == (1, 3) and not one.any()


@pytest.mark.parametrize('scale', [3.7, 2.0 ** -20, 1e6])
def test_normals_at_odd_and_tiny_extents(scale):
    v, f = random_mesh(41, 300, 700, scale)
    n = check_normals(v, f)
    length = np.linalg.norm(n.astype(np.float64), axis=1)
    assert (np.abs(length[length > 0] - 1) < 1e-6).all()


# ---------------------------------------------------------------- interpolation and shade
def run_interp(face, v, f32, cams, near, attr=None, fill=0.0, shade_mode=0, normals=None):
    """hip.mesh_interp twice into padded buffers -> (attr float32 [B,H,W,C] or None, shade float32 [B,H,W] or None)"""
    B, Hh, Ww = face.shape
    fd, vd, qd, cd = dev(face), dev(v), dev(f32), dev(cams)
    ad, nd = None if attr is None else dev(attr), None if normals is None else dev(normals)
    res = []
    for _ in range(2):
        oa = None if attr is None else Padded((B, Hh, Ww, attr.shape[1]), torch.float32)
        os_ = None if shade_mode == 0 else Padded((B, Hh, Ww), torch.float32)
        hip.mesh_interp(fd, vd, qd, cd, near, attr=ad, fill=fill, out_attr=None if oa is None else oa.t, shade_mode=shade_mode, normals=nd,
                        out_shade=None if os_ is None else os_.t)
        torch.cuda.synchronize()
        assert (oa is None or oa.intact()) and (os_ is None or os_.intact())
        res.append((None if oa is None else oa.t.cpu().numpy(), None if os_ is None else os_.t.cpu().numpy()))
    for a, b in zip(*res):
        assert (a is None and b is None) or np.array_equal(bits(a), bits(b))
    return res[0]


def assert_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(bits(got), bits(want)), (what, int((bits(got) != bits(want)).sum()))


SHAPE, NEAR = (37, 51), 0.05


@functools.lru_cache(maxsize=None)
def scene_case():
    """the mesh tests' scene from three cameras with fx != fy: the device render's face map and the restatement's outputs, computed once"""
    sc = M.scene()
    v = sc['vertices']
    f32 = faces32(sc['faces'], len(v))
    cams2world = sc['cams'][:3]
    focals = [[M.focal_of(SHAPE), 1.25 * M.focal_of(SHAPE)]]
    tab = M.camera_table(cams2world, focals, SHAPE)
    assert np.array_equal(bits(mesh_camera_table(cams2world, focals, SHAPE)), bits(tab))
    r = render_mesh(dev(v), dev(sc['faces']), cams2world, focals, SHAPE, near=NEAR)
    face = r.face.cpu().numpy()
    assert (face >= 0).mean() > 0.5 and (face < 0).any()
    rng = np.random.default_rng(51)
    attr = rng.uniform(-2, 2, (len(v), 16)).astype(F)
    attr[:, 1] = np.nan_to_num(v[:, 2])
    nrm = S.normals(v, sc['faces'])
    smooth = S.interp(face, v, sc['faces'], tab, NEAR, attr=attr, fill=-1.0, shade_mode=2, normals=nrm)
    flat = S.interp(face, v, sc['faces'], tab, NEAR, shade_mode=1)
    assert np.array_equal(smooth['hit'], face >= 0) and (smooth['shade'][face >= 0] > 0).any() and (flat['shade'][face >= 0] > 0).all()
    return dict(v=v, f32=f32, faces=sc['faces'], cams2world=cams2world, focals=focals, tab=tab, face=face, attr=attr, normals=nrm, smooth=smooth, flat=flat)


@pytest.mark.parametrize('C', [1, 3, 4, 16])
def test_attributes_and_smooth_shade_over_a_rendered_map(C):
    c = scene_case()
    attr = np.ascontiguousarray(c['attr'][:, :C])
    got_a, got_s = run_interp(c['face'], c['v'], c['f32'], c['tab'], NEAR, attr=attr, fill=-1.0, shade_mode=2, normals=c['normals'])
    assert_bits(got_a, np.ascontiguousarray(c['smooth']['attr'][..., :C]), 'attr')
    assert_bits(got_s, c['smooth']['shade'], 'smooth shade')
    assert (got_a[c['face'] < 0] == F(-1)).all() and (got_s[c['face'] < 0] == 0).all()
    only_a, none = run_interp(c['face'], c['v'], c['f32'], c['tab'], NEAR, attr=attr, fill=-1.0)        # attributes alone
    assert none is None
    assert_bits(only_a, got_a, 'attr alone')


def test_flat_shade_and_the_public_entry_points_over_a_rendered_map():
    c = scene_case()
    none, got = run_interp(c['face'], c['v'], c['f32'], c['tab'], NEAR, shade_mode=1)
    assert none is None
    assert_bits(got, c['flat']['shade'], 'flat shade')
    vd, fd, face = dev(c['v']), dev(c['faces']), dev(c['face'])
    assert_bits(shade_render(face, vd, fd, c['cams2world'], c['focals'], near=NEAR).cpu().numpy(), c['flat']['shade'], 'shade_render flat')
    assert_bits(shade_render(face, vd, fd, c['cams2world'], c['focals'], normals=dev(c['normals']), near=NEAR).cpu().numpy(), c['smooth']['shade'], 'shade_render smooth')
    got = interpolate_render(face, vd, fd, c['cams2world'], c['focals'], dev(c['attr'][:, :3].copy()), near=NEAR, fill=-1.0)
    assert_bits(got.cpu().numpy(), np.ascontiguousarray(c['smooth']['attr'][..., :3]), 'interpolate_render')
    depth = interpolate_render(face, vd, fd, c['cams2world'], c['focals'], dev(c['attr'][:, 1:2].copy()), near=NEAR)[..., 0]
    want = render_mesh(vd, fd, c['cams2world'], c['focals'], SHAPE, near=NEAR).depth
    assert float((depth[0] - want[0]).abs().max()) < 1e-5                      # camera 0 is the identity: there 'z of the vertex' is the depth (to rounding at generic depths)


H2, W2, F2, PP2 = 5, 7, 4.0, (3.5, 2.5)


def at2(u, v, z):
    return [(u - PP2[0]) * z / F2, (v - PP2[1]) * z / F2, z]


@functools.lru_cache(maxsize=None)
def hand_case():
    """two 5 x 7 cameras and a mesh of four faces: 0 a small face (A > 0), 1 a face listed with A < 0 (the exchange) with three distinct attribute rows,
    2 a face behind `near`, 3 a floor triangle that fills the image of camera 0.  The maps are made by hand."""
    v = np.array([at2(0.5, 0.5, 1.5), at2(3.5, 0.75, 2.5), at2(0.75, 3.5, 3.5),                    # face 0
                  at2(3.0, 1.0, 2.0), at2(3.25, 4.75, 3.0), at2(6.75, 1.25, 5.0),                  # face 1: A < 0 as listed
                  at2(1.0, 1.0, 0.01), at2(5.0, 1.0, 0.01), at2(1.0, 4.0, 0.01),                   # face 2: nearer than near
                  at2(-8.0, -6.0, 6.0), at2(24.0, -6.0, 7.0), at2(-8.0, 18.0, 9.0)], dtype=F)      # face 3: fills the image
    f = np.arange(12, dtype=np.int64).reshape(4, 3)
    shift = np.eye(4)
    shift[:3, 3] = [0.4, -0.3, -0.5]
    cams2world = [np.eye(4), shift]
    tab = M.camera_table(cams2world, [[F2, F2]], (H2, W2), [PP2])
    face = np.full((2, H2, W2), 3, dtype=np.int64)
    face[0, 0, :4] = [-1, 4, 2 ** 32 - 1, -7]                                  # no face at all
    face[0, 3, :3] = 2                                                         # behind near: not drawn
    face[0, 4, 5:] = 0                                                         # face 0 does not reach the far corner
    face[0, 1:3, 1] = 0
    face[0, 1:3, 4] = 1
    face[1, :2] = 1
    face[1, 4, :] = [0, 0, -1, 3, 3, 2, 1]
    attr = np.random.default_rng(61).uniform(0, 1, (12, 3)).astype(F)
    nrm = S.normals(v, f)
    want = S.interp(face, v, f, tab, NEAR, attr=attr, fill=-1.0, shade_mode=2, normals=nrm)
    hit = want['hit']
    assert not hit[0, 0, :4].any() and not hit[0, 3, :3].any() and not hit[0, 4, 5:].any() and hit[0, 1:3, 1].all() and hit[0, 1:3, 4].all()
    full = np.full((1, H2, W2), 3, dtype=np.int64)
    assert S.interp(full, v, f, tab[:1], NEAR, shade_mode=1)['hit'].all()       # the floor fills camera 0
    s0 = M.setup(v, f, tab[0], H2, W2, NEAR)
    assert list(s0['swapped']) == [False, True, False, False] and list(s0['ok']) == [True, True, False, True]
    return dict(v=v, f=f, tab=tab, face=face, attr=attr, normals=nrm, want=want)


def test_cameras_in_chunks(monkeypatch):
    """a budget of one camera per launch: the slices of the face map, the camera table and both outputs at b0 > 0"""
    from panst3r_amd.engine import shade as shade_mod
    c = scene_case()
    monkeypatch.setattr(shade_mod, 'ZBUF_BYTES', 8 * SHAPE[0] * SHAPE[1])
    assert shade_mod.chunk_step(3, SHAPE[0], SHAPE[1], shade_mod.ZBUF_BYTES) == 1
    calls = []
    monkeypatch.setattr(hip, 'mesh_interp', lambda face, *a, _f=hip.mesh_interp, **k: (calls.append(face.shape[0]), _f(face, *a, **k))[1])
    col, shade = shade_mod.color_and_shade(dev(c['face']), dev(c['v']), dev(c['faces']), c['cams2world'], c['focals'], dev(c['attr'][:, :3].copy()),
                                           normals=dev(c['normals']), near=NEAR)
    assert calls == [1, 1, 1]
    want = S.interp(c['face'], c['v'], c['faces'], c['tab'], NEAR, attr=np.ascontiguousarray(c['attr'][:, :3]), fill=0.0, shade_mode=2, normals=c['normals'])
    assert_bits(col.cpu().numpy(), want['attr'], 'attr in chunks')
    assert_bits(shade.cpu().numpy(), want['shade'], 'shade in chunks')
    assert (shade[1:].cpu().numpy()[c['face'][1:] >= 0] > 0).any()


def test_hand_made_maps():
    c = hand_case()
    f32 = faces32(c['f'], len(c['v']))
    got_a, got_s = run_interp(c['face'], c['v'], f32, c['tab'], NEAR, attr=c['attr'], fill=-1.0, shade_mode=2, normals=c['normals'])
    assert_bits(got_a, c['want']['attr'], 'attr')
    assert_bits(got_s, c['want']['shade'], 'smooth shade')
    miss = ~c['want']['hit']
    assert (got_a[miss] == F(-1)).all() and (got_s[miss] == 0).all() and miss.sum() >= 9
    wrong = S.interp(c['face'], c['v'], c['f'], c['tab'], NEAR, attr=c['attr'], fill=-1.0, variant='no_swap')['attr']
    assert not np.array_equal(wrong[0, 1:3, 4], got_a[0, 1:3, 4])             # the exchange shows on these pixels
    _, flat = run_interp(c['face'], c['v'], f32, c['tab'], NEAR, shade_mode=1)
    assert_bits(flat, S.interp(c['face'], c['v'], c['f'], c['tab'], NEAR, shade_mode=1)['shade'], 'flat shade')


@pytest.mark.parametrize('npix', [255, 256, 257])
def test_the_launch_edges_of_the_pixel_kernel(npix):
    v = np.array([[-40.0, -1.0, 1.0], [80.0, -1.5, 2.0], [0.0, 3.0, 1.5]], dtype=F)      # one face over the whole 1 x npix strip
    f = np.array([[0, 1, 2]])
    tab = M.camera_table([np.eye(4)], [[8.0, 8.0]], (1, npix), [(npix / 2, 0.5)])
    face = np.zeros((1, 1, npix), dtype=np.int64)
    face[0, 0, 5] = -1
    attr = np.random.default_rng(npix).uniform(0, 1, (3, 2)).astype(F)
    want = S.interp(face, v, f, tab, NEAR, attr=attr, fill=0.5, shade_mode=1)
    assert want['hit'].sum() == npix - 1 and want['hit'][0, 0, -1]
    got_a, got_s = run_interp(face, v, faces32(f, 3), tab, NEAR, attr=attr, fill=0.5, shade_mode=1)
    assert_bits(got_a, want['attr'], 'attr')
    assert_bits(got_s, want['shade'], 'flat shade')


# ---------------------------------------------------------------- refusals
def test_refusals_leave_the_outputs_untouched():
    c = hand_case()
    B = 2
    v, f, cams, face = dev(c['v']), dev(faces32(c['f'], 12)), dev(c['tab']), dev(c['face'])
    attr, nrm = dev(c['attr']), dev(c['normals'])
    oa, os_ = Padded((B, H2, W2, 3), torch.float32), Padded((B, H2, W2), torch.float32)
    ok = dict(attr=attr, fill=0.0, out_attr=oa.t, shade_mode=2, normals=nrm, out_shade=os_.t)
    wide, o17 = torch.zeros(12, 17, device=DEV), Padded((B, H2, W2, 17), torch.float32)
    empty, o0 = torch.zeros(12, 0, device=DEV), Padded((B, H2, W2, 0), torch.float32)
    cases = [
        ('a CPU face map', dict(face=face.cpu())), ('CPU vertices', dict(vertices=v.cpu())), ('CPU attributes', dict(attr=attr.cpu())),
        ('an int32 face map', dict(face=face.int())), ('float64 attributes', dict(attr=attr.double())), ('int64 faces', dict(faces=f.long())),
        ('float64 vertices', dict(vertices=v.double())), ('a short camera table', dict(cams=cams[:1])), ('a 2-D face map', dict(face=face[0])),
        ('an output of the wrong shape', dict(out_attr=oa.t[:1])), ('a shade output of the wrong shape', dict(out_shade=os_.t[0])),
        ('17 channels', dict(attr=wide, out_attr=o17.t)), ('no channel', dict(attr=empty, out_attr=o0.t)),
        ('attributes of another mesh', dict(attr=attr[:11].contiguous())), ('normals of another mesh', dict(normals=nrm[:11].contiguous())),
        ('smooth shade without normals', dict(normals=None)), ('normals without the smooth mode', dict(shade_mode=1)),
        ('a shade output without a mode', dict(shade_mode=0, normals=None)), ('attributes without an output', dict(out_attr=None)),
        ('an unknown shade mode', dict(shade_mode=3)), ('a NaN fill', dict(fill=float('nan'))), ('an infinite fill', dict(fill=float('inf'))),
        ('a fill beyond float32', dict(fill=1e39)), ('a near of zero', dict(near=0.0)),
    ]
    for what, change in cases:
        pos = dict(face=face, vertices=v, faces=f, cams=cams, near=NEAR)
        kw = dict(ok)
        for k, x in change.items():
            (pos if k in pos else kw)[k] = x
        with pytest.raises(RuntimeError):
            hip.mesh_interp(pos['face'], pos['vertices'], pos['faces'], pos['cams'], pos['near'], **kw)
            pytest.fail('mesh_interp accepted ' + what)
        torch.cuda.synchronize()
        assert oa.untouched() and os_.untouched() and o17.untouched() and o0.untouched(), what
    with pytest.raises(RuntimeError):
        hip.mesh_interp(face, v, f, cams, NEAR)                                # nothing asked for
    acc, out = Padded((12, 3, 2), torch.int64), Padded((12, 3), torch.float32)
    for what, args in [('CPU vertices', (v.cpu(), f, 0, acc.t, out.t)), ('int64 faces', (v, f.long(), 0, acc.t, out.t)), ('a short acc', (v, f, 0, acc.t[:11], out.t)),
                       ('a short output', (v, f, 0, acc.t, out.t[:11])), ('sh out of range', (v, f, 1101, acc.t, out.t)), ('a float sh', (v, f, 1.0, acc.t, out.t)),
                       ('an int32 acc', (v, f, 0, acc.t.int(), out.t))]:
        with pytest.raises(RuntimeError):
            hip.mesh_normals(*args)
            pytest.fail('mesh_normals accepted ' + what)
        torch.cuda.synchronize()
        assert acc.untouched() and out.untouched(), what
    for bad in (dict(attributes=attr.cpu()), dict(attributes=torch.zeros(12, 17, device=DEV)), dict(attributes=attr[:11]), dict(fill=float('nan'))):
        kw = dict(attributes=attr, fill=0.0)
        kw.update(bad)
        with pytest.raises((RuntimeError, ValueError)):
            interpolate_render(face, v, f, [np.eye(4)] * 2, F2, kw['attributes'], pp=PP2, fill=kw['fill'])
    with pytest.raises((RuntimeError, ValueError)):
        shade_render(face, v, f, [np.eye(4)] * 2, F2, normals=nrm[:11], pp=PP2)
    with pytest.raises((RuntimeError, ValueError)):
        shade_render(face, v, f, [np.eye(4)] * 3, F2, pp=PP2)                  # three cameras for two views
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        vertex_normals(v.cpu(), f.cpu())


# ---------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def room():
    import test_hip_surface as TS                                              # the seeded room of the surface tests, built once per process
    return TS.device_cloud().mesh(), TS.source_views()


@pytest.mark.parametrize('shading', ['smooth', 'flat', None])
def test_render_color_equals_the_restatement(shading):
    mesh, views = room()
    v, f, col = mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy().astype(np.int64), mesh.colors.cpu().numpy()
    assert np.array_equal(bits(mesh.vertex_normals()), bits(S.normals(v, f))) and mesh.vertex_normals() is mesh.vertex_normals()
    assert mesh.drop_small(2)._normals is None                                 # a mesh with other faces computes its own
    for k, (c2w, focal, shape) in enumerate(views):
        background = (0.25, 0.5, 1.0) if k else (0, 0, 0)
        r, rgb = mesh.render_color([c2w], focal, shape, shading=shading, background=background)
        assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (1,) + tuple(shape) + (3,)
        face = r.face.cpu().numpy()
        want = S.render_color(face, v, f, M.camera_table([c2w], focal, shape), NEAR, col, shading, 0.3, background)
        assert (face >= 0).sum() > 50 and (face < 0).any() and np.array_equal(rgb.cpu().numpy(), want)
        assert (rgb.cpu().numpy()[face < 0] == S.colors_u8(np.asarray(background, dtype=F))).all()
    palette = torch.rand(len(mesh.vertices), 3, generator=torch.Generator().manual_seed(1)).to(DEV)
    c2w, focal, shape = views[0]
    r, rgb = mesh.render_color([c2w], focal, shape, colors=palette, shading=shading, ambient=0.5)
    want = S.render_color(r.face.cpu().numpy(), v, f, M.camera_table([c2w], focal, shape), NEAR, palette.cpu().numpy(), shading, 0.5)
    assert np.array_equal(rgb.cpu().numpy(), want)


def test_an_empty_mesh_renders_as_background():
    mesh, views = room()
    empty = mesh._with_faces(mesh.faces[:0], mesh.face_ids[:0], mesh.quad[:0])
    c2w, focal, shape = views[0]
    r, rgb = empty.render_color([c2w], focal, shape, background=(1.0, 0.5, 0.0))
    assert not r.hit.any() and tuple(rgb.shape) == (1,) + tuple(shape) + (3,) and (rgb.cpu().numpy() == np.array([255, 128, 0], dtype=np.uint8)).all()
    assert not empty.vertex_normals().any()


def test_ply_with_normals_and_the_default_file(tmp_path):
    mesh = room()[0].drop_small(2)
    plain, again = mesh.write_ply(str(tmp_path / 'a.ply')), mesh.write_ply(str(tmp_path / 'b.ply'), normals=False)
    assert open(plain, 'rb').read() == open(again, 'rb').read()
    path = mesh.write_ply(str(tmp_path / 'n.ply'), normals=True)
    raw, raw0 = open(path, 'rb').read(), open(plain, 'rb').read()
    for p in (plain, path):                                                    # load_ply_mesh reads both forms
        v, f = load_ply_mesh(p)
        assert np.array_equal(bits(v), bits(mesh.vertices)) and np.array_equal(f.numpy(), mesh.faces.cpu().numpy().astype(np.int64))
    head = raw[:raw.index(b'end_header\n') + 11]
    assert b'property float nx\nproperty float ny\nproperty float nz\nelement face' in head and b'property float nx' not in raw0[:raw0.index(b'end_header\n')]
    Mv, Fn = len(mesh.vertices), len(mesh)
    body, body0 = raw[len(head):], raw0[raw0.index(b'end_header\n') + 11:]
    assert len(body) == 31 * Mv + 17 * Fn and len(body0) == 19 * Mv + 17 * Fn and body[31 * Mv:] == body0[19 * Mv:]
    vert = np.frombuffer(body, dtype=np.dtype([('xyz', '<f4', (3,)), ('rgb', 'u1', (3,)), ('label', '<i4'), ('n', '<f4', (3,))]), count=Mv)
    vert0 = np.frombuffer(body0, dtype=np.dtype([('xyz', '<f4', (3,)), ('rgb', 'u1', (3,)), ('label', '<i4')]), count=Mv)
    assert np.array_equal(bits(vert['n']), bits(mesh.vertex_normals())) and np.array_equal(vert['rgb'], vert0['rgb']) and np.array_equal(vert['label'], vert0['label'])
    assert np.array_equal(bits(vert['n']), bits(S.normals(mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy().astype(np.int64))))
