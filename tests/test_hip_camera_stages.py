"""Stage-level parity of csrc/render.hip (render_splat, render_resolve) and csrc/mesh.hip (mesh_raster, mesh_resolve, mesh_area_count, mesh_area_apply)
at the DECISION EDGES of their contract: every wrapper of panst3r_amd.hip called by hand on tensors built from numpy, the z-buffer itself (uint64) and
then every resolve output compared BIT FOR BIT with the yardsticks (render_ref.splat / resolve, mesh_ref.setup / raster / resolve, per camera) on the
constructed cases of tests/camera_stage_cases.py.  No tolerance and no cap; every output is allocated with canary padding that must survive.  Every
splat / raster case runs with `precheck` 0 and 1.  tests/test_camera_stage_checks.py asserts without a GPU that each case holds what it was built for
and that every planted mistake changes a named case.

  splat    pixel rule (an integer u and one ulp below, -0.0, (-1, 0) at radius 0 and 1, u = W; the same in v) | cull (zc == near and one ulp below,
           non-finite and negative zc, xc / yc non-finite, an overflow inside the rotated pose) | limit (u, v == 2^20 on a 2^20 + 2 wide / high image, the
           next fp32 dropped) | footprint (an integer quotient and one ulp below, radius against the point-size radius, max_radius, a +inf quotient,
           half_size 0, clipping on four sides, the fp32 product) | depth and ties (rows of two workgroups, one ulp of depth, rows 1, 3, 4) | launch
           edges (M around 256, three different cameras, 65 535 cameras)
  resolve  render_resolve on hand-made buffers of 255, 256, 257 cells: empty, row M - 1, rows >= M (empty by the contract), arbitrary depth bits
  raster   the top-left rule (split quads, the strip) | snap (half-way vertices of each class) | planes (depth == near / far, a corner at near) | limit
           (u, v == 2^14) | bad faces | nearest corner (ties in four listings, a clockwise face) | depth (the association of the three-term sum) |
           duplicate faces of two workgroups | the two paths (boxes of 64 and 65 pixels, capacities around the number of large entries) | the stride
           loop of the wave path (10 245 entries) | launch edges (Nf around 256, three different cameras)
  resolve  mesh_resolve on hand-made buffers: empty, face >= Nf, a face that is not rasterised in that camera, the camera boundary at H W = 35
  area     runs of 63 .. 257 pixels across wave, workgroup and camera edges, ids and table entries at and outside their ranges, min_area exactly met
  refusals one call per rule of each wrapper: it raises and writes nothing

Every index a kernel reads stays inside a tensor of the test; the only refusals exercised are the launchers' own, made on the host before any launch."""
import numpy as np
import pytest
import torch

import camera_stage_cases as C
import render_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F = np.float32
CANARY_I, CANARY_F = -12345, -777.0
PAD = 64                                    # canary elements behind every output
M_LANE = 64                                 # PST_MESH_LANE_PIXELS: a larger bounding box goes to the wave path


def _hip():
    from panst3r_amd import hip
    hip.lib()
    return hip


def _dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).to(DEV).contiguous()


def _filled(shape, dtype):
    return torch.full(shape, CANARY_F if dtype == torch.float32 else CANARY_I, dtype=dtype, device=DEV)


def _untouched(t):
    return bool((t == (CANARY_F if t.dtype == torch.float32 else CANARY_I)).all())


def _assert_same(got, ref, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    ref = np.asarray(ref)
    assert got.dtype == ref.dtype, (what, got.dtype, ref.dtype)
    assert C.same_bits(got.reshape(ref.shape), ref), '%s: %s' % (what, C.first_difference(got.reshape(ref.shape), ref))


def _cells(B, H, W, fill=-1):
    """-> (the whole allocation, zbuf int64 [B, H, W] inside it, filled with all ones); PAD canary cells follow the buffer"""
    n = B * H * W
    buf = _filled((n + PAD,), torch.int64)
    buf[:n] = fill
    return buf, buf[:n].view(B, H, W)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _padded(n, dtype, inner=()):
    buf = _filled((n + PAD,) + inner, dtype)
    return buf, buf[:n]


# ------------------------------------------------------------------------------------------------------------------------------------------ splatter
def _splat(hip, case, precheck, pts=None, cams=None):
    B, H, W = len(case['cams']), case['H'], case['W']
    buf, zbuf = _cells(B, H, W)
    hip.render_splat(_dev(case['points']) if pts is None else pts, _dev(case['cams']) if cams is None else cams, H, W, float(case['half']), case['radius'],
                     case['max_radius'], zbuf, precheck=precheck)
    torch.cuda.synchronize()
    assert _untouched(buf[B * H * W:]), 'render_splat wrote past the buffer'
    return zbuf


def _render_resolve(hip, zbuf, M_, want_from):
    """resolve the device cells `zbuf` over a cloud of M_ rows that name themselves; compare with render_ref.resolve of the uint64 cells `want_from`"""
    rgb, colors, pan = C.cloud_fields(M_)
    n = zbuf.numel()
    out = {'index': _padded(n, torch.int64), 'depth': _padded(n, torch.float32), 'pan': _padded(n, torch.int32), 'rgb': _padded(n, torch.float32, (3,)),
           'colors': _padded(n, torch.float32, (3,))}
    hip.render_resolve(zbuf, _dev(rgb), _dev(colors), _dev(pan), *(out[k][1] for k in ('index', 'depth', 'pan', 'rgb', 'colors')))
    torch.cuda.synchronize()
    want = dict(zip(('index', 'depth', 'pan', 'rgb', 'colors'), R.resolve(want_from, rgb, colors, pan)))
    for k, (buf, t) in out.items():
        _assert_same(t, want[k], k)
        assert _untouched(buf[n:]), k + ': written past the last cell'
    return {k: t.cpu().numpy() for k, (buf, t) in out.items()}


def _splat_group(group):
    hip = _hip()
    for name, case in C.splat_cases()[group].items():
        want = C.splat_zbuf(case)
        pts, cams = _dev(case['points']), _dev(case['cams'])
        for precheck in (0, 1):
            zbuf = _splat(hip, case, precheck, pts, cams)
            _assert_same(_u64(zbuf).reshape(want.shape), want, 'zbuf of %s/%s (precheck=%d)' % (group, name, precheck))
        _render_resolve(hip, zbuf, len(case['points']), want.reshape(-1))


def test_splat_pixel_rule():
    _splat_group('pixel')


def test_splat_cull():
    _splat_group('cull')


def test_splat_limit_on_an_image_2_20_wide_and_high():
    _splat_group('limit')


def test_splat_footprint():
    _splat_group('footprint')


def test_splat_depth_and_ties():
    _splat_group('depth')


def test_splat_launch_edges():
    _splat_group('launch')


def test_splat_65535_cameras():
    hip = _hip()
    case, want = C.many_cameras()
    for precheck in (0, 1):
        zbuf = _splat(hip, case, precheck)
        _assert_same(_u64(zbuf).reshape(want.shape), want, 'zbuf (precheck=%d)' % precheck)


def test_splat_twice_gives_identical_bytes():
    hip = _hip()
    case = C.splat_cases()['launch']['rotated']
    a, b = (_u64(_splat(hip, case, 1)).tobytes() for _ in range(2))
    assert a == b


@pytest.mark.parametrize('npix', [255, 256, 257])
def test_render_resolve_on_hand_made_cells(npix):
    hip = _hip()
    z = C.render_resolve_case(npix)
    buf, zbuf = _cells(1, 1, npix)
    zbuf.copy_(_dev(z.view(np.int64)).view(1, 1, npix))
    got = _render_resolve(hip, zbuf, C.RESOLVE_M, z)
    assert (got['index'][[0, 2, 3]] == -1).all() and got['index'][1] == C.RESOLVE_M - 1 and got['index'][npix - 1] == C.RESOLVE_M - 1
    assert C.bits1(got['depth'][4]) == 0x7FC00001 and C.bits1(got['depth'][6]) == 0x80000000


# ---------------------------------------------------------------------------------------------------------------------------------------- rasteriser
def _raster(hip, case, capacity, precheck, dev=None):
    """-> (zbuf int64 [B, H, W] on the device, the number of appends to the list of large faces)"""
    B, H, W, Nf = len(case['cams']), case['H'], case['W'], len(case['faces'])
    v, f, cams = dev if dev is not None else (_dev(case['vertices']), _dev(case['faces']), _dev(case['cams']))
    cap = B * Nf if capacity is None else capacity
    ws = {'big': _filled((cap + PAD,), torch.int64), 'count': torch.zeros(1, dtype=torch.int64, device=DEV), 'capacity': cap}
    buf, zbuf = _cells(B, H, W)
    hip.mesh_raster(v, f, cams, H, W, float(case['near']), float(case['far']), zbuf, ws, precheck=precheck)
    torch.cuda.synchronize()
    assert _untouched(buf[B * H * W:]), 'mesh_raster wrote past the buffer'
    assert _untouched(ws['big'][cap:]), 'mesh_raster wrote past the list of large faces'
    return zbuf, int(ws['count'].cpu()[0]), ws['big'][:cap].cpu().numpy()


def _mesh_resolve(hip, case, zbuf, want_from, setups, dev=None):
    """every kind of id the case has, on the device cells `zbuf`, against mesh_ref.resolve of the uint64 cells `want_from` [B, H W]"""
    v, f, cams = dev if dev is not None else (_dev(case['vertices']), _dev(case['faces']), _dev(case['cams']))
    n = zbuf.numel()
    for kind in ('vertex', 'face', 'none'):
        if kind != 'none' and case[kind + '_ids'] is None:
            continue
        out = {'face': _padded(n, torch.int64), 'depth': _padded(n, torch.float32), 'pan': _padded(n, torch.int32)}
        hip.mesh_resolve(zbuf, v, f, cams, float(case['near']), _dev(case['vertex_ids']) if kind == 'vertex' else None,
                         _dev(case['face_ids']) if kind == 'face' else None, *(out[k][1] for k in ('face', 'depth', 'pan')))
        torch.cuda.synchronize()
        want = dict(zip(('face', 'depth', 'pan'), C.mesh_resolved(case, want_from, kind, setups=setups)))
        for k, (buf, t) in out.items():
            _assert_same(t, want[k].reshape(-1), '%s (%s ids)' % (k, kind))
            assert _untouched(buf[n:]), k + ': written past the last cell'


def _mesh_case(hip, case, what):
    setups = C.mesh_setups(case)
    want = C.mesh_zbuf(case, setups=setups)
    large = int(sum((s['box'] > M_LANE).sum() for s in setups))
    dev = (_dev(case['vertices']), _dev(case['faces']), _dev(case['cams']))
    for capacity in case['capacities']:
        for precheck in (0, 1):
            zbuf, count, big = _raster(hip, case, capacity, precheck, dev)
            _assert_same(_u64(zbuf).reshape(want.shape), want, 'zbuf of %s (capacity=%s, precheck=%d)' % (what, capacity, precheck))
            assert count == large, (what, capacity, count, large)                # every large face asks for a slot, whatever the capacity
            listed = big[:min(count, len(big))]
            assert len(set(listed.tolist())) == len(listed), 'an entry is listed twice'
    _mesh_resolve(hip, case, zbuf, want, setups, dev)
    return large



def _mesh_group(group):
    hip = _hip()
    assert hip.mesh_lane_pixels() == M_LANE
    for name, case in C.mesh_cases()[group].items():
        _mesh_case(hip, case, group + '/' + name)


def test_raster_top_left_rule():
    _mesh_group('topleft')


def test_raster_snap():
    _mesh_group('snap')


def test_raster_planes():
    _mesh_group('planes')


def test_raster_limit():
    _mesh_group('limit')


def test_raster_bad_faces():
    _mesh_group('bad')


def test_raster_nearest_corner():
    _mesh_group('corner')


def test_raster_depth_association():
    _mesh_group('depth')


def test_raster_duplicate_faces():
    _mesh_group('duplicate')


def test_raster_two_paths():
    hip = _hip()
    case = C.mesh_cases()['paths']['boxes']
    assert _mesh_case(hip, case, 'paths/boxes') == case['capacities'][0]       # the first capacity is exactly the number of large entries
    _mesh_case(hip, C.mesh_cases()['paths']['rotated'], 'paths/rotated')


def test_raster_stride_loop_of_the_wave_path():
    hip = _hip()
    case = C.stride_case()
    assert _mesh_case(hip, case, 'stride') == C.STRIDE_H * C.STRIDE_B > C.BIG_WAVES


def test_raster_launch_edges():
    _mesh_group('launch')


def test_raster_twice_gives_identical_bytes():
    hip = _hip()
    case = C.mesh_cases()['launch']['rotated']
    a, b = (_u64(_raster(hip, case, None, 0)[0]).tobytes() for _ in range(2))
    assert a == b


def test_mesh_resolve_on_hand_made_cells():
    hip = _hip()
    case, z = C.mesh_resolve_case()
    B, H, W = 2, case['H'], case['W']
    buf, zbuf = _cells(B, H, W)
    zbuf.copy_(_dev(z.view(np.int64)).view(B, H, W))
    _mesh_resolve(hip, case, zbuf, z, C.mesh_setups(case))


# ---------------------------------------------------------------------------------------------------------------------------------------------- area
@pytest.mark.parametrize('min_area', [C.AREA_MIN, 0])
@pytest.mark.parametrize('name', list(C.area_cases()))
def test_area_count_and_apply(name, min_area):
    hip = _hip()
    pan = C.area_cases()[name]
    B, hw = pan.shape
    want_counts, want_out = C.area_ref(pan, C.AREA_ID2ROW, C.AREA_S, min_area)
    d_pan, d_tab = _dev(pan.reshape(B, 1, hw)), _dev(C.AREA_ID2ROW)
    cbuf = _filled((B * C.AREA_S + PAD,), torch.int32)
    counts = cbuf[:B * C.AREA_S].view(B, C.AREA_S)
    counts.zero_()
    obuf = _filled((B * hw + PAD,), torch.int32)
    out = obuf[:B * hw].view(B, 1, hw)
    hip.mesh_area_count(d_pan, d_tab, counts)
    hip.mesh_area_apply(d_pan, d_tab, counts, min_area, out)
    torch.cuda.synchronize()
    _assert_same(counts, want_counts, 'counts of ' + name)
    _assert_same(out, want_out.reshape(B, 1, hw), 'out of ' + name)
    assert _untouched(cbuf[B * C.AREA_S:]) and _untouched(obuf[B * hw:])


# ----------------------------------------------------------------------------------------------------------------------------------------- refusals
def test_render_refusals_write_nothing():
    hip = _hip()
    case = C.splat_cases()['launch']['M_257']
    pts, cams = _dev(case['points']), _dev(case['cams'])
    buf, zbuf = _cells(1, 6, 8, fill=CANARY_I)
    ok = dict(points=pts, cams=cams, H=6, W=8, half_size=0.25, radius=1, max_radius=4, zbuf=zbuf)
    many = torch.zeros(65536, 16, dtype=torch.float32, device=DEV)
    mbuf, mz = _cells(65536, 1, 1, fill=CANARY_I)
    for bad in (dict(cams=many, H=1, W=1, zbuf=mz), dict(radius=17), dict(max_radius=17), dict(radius=-1), dict(half_size=float('nan')), dict(half_size=-0.5),
                dict(half_size=float('inf')), dict(points=pts[:0])):
        with pytest.raises(RuntimeError, match='render_splat'):
            hip.render_splat(**dict(ok, **bad))
    rgb, colors, pan = (_dev(t) for t in C.cloud_fields(257))
    out = [_filled((48,), torch.int64), _filled((48,), torch.float32), _filled((48,), torch.int32), _filled((48, 3), torch.float32), _filled((48, 3), torch.float32)]
    with pytest.raises(RuntimeError, match='render_resolve'):
        hip.render_resolve(zbuf, rgb[:0], colors[:0], pan[:0], *out)           # M = 0
    torch.cuda.synchronize()
    assert _untouched(buf) and _untouched(mbuf) and all(_untouched(t) for t in out)


def test_mesh_refusals_write_nothing():
    hip = _hip()
    case = C.mesh_cases()['launch']['Nf_257']
    v, f, cams = _dev(case['vertices']), _dev(case['faces']), _dev(case['cams'])
    H, W = case['H'], case['W']
    buf, zbuf = _cells(1, H, W, fill=CANARY_I)
    ws = {'big': _filled((257,), torch.int64), 'count': torch.zeros(1, dtype=torch.int64, device=DEV), 'capacity': 257}
    for near, far in ((1.0, 1.0), (2.0, 1.0), (0.0, 1.0), (-1.0, 1.0), (0.5, float('inf')), (float('nan'), 1.0)):
        with pytest.raises(RuntimeError, match='mesh_raster'):
            hip.mesh_raster(v, f, cams, H, W, near, far, zbuf, ws)
    many = torch.zeros(65536, 16, dtype=torch.float32, device=DEV)
    mbuf, mz = _cells(65536, 1, 1, fill=CANARY_I)
    with pytest.raises(RuntimeError, match='mesh_raster'):
        hip.mesh_raster(v, f, many, 1, 1, 0.5, 10.0, mz, ws)
    with pytest.raises(RuntimeError, match='mesh_raster'):                     # big_capacity < 0: the wrapper's own assertion stands in front of it
        hip._call('pst_mesh_raster', v.data_ptr(), v.shape[0], f.data_ptr(), f.shape[0], cams.data_ptr(), 1, H, W, 0.5, 10.0, zbuf.data_ptr(), ws['big'].data_ptr(),
                  ws['count'].data_ptr(), -1, 0)
    n = H * W
    out = [_filled((n,), torch.int64), _filled((n,), torch.float32), _filled((n,), torch.int32)]
    with pytest.raises(RuntimeError, match='exclusive'):
        hip.mesh_resolve(zbuf, v, f, cams, 0.5, _dev(np.ones(len(case['vertices']), np.int32)), _dev(case['face_ids']), *out)
    mout = [_filled((65536,), torch.int64), _filled((65536,), torch.float32), _filled((65536,), torch.int32)]
    with pytest.raises(RuntimeError, match='mesh_resolve'):
        hip.mesh_resolve(mz, v, f, many, 0.5, None, None, *mout)
    torch.cuda.synchronize()
    assert _untouched(buf) and _untouched(mbuf) and _untouched(ws['big']) and int(ws['count'].cpu()[0]) == 0 and all(_untouched(t) for t in out + mout)
