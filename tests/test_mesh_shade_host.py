"""The mesh shading contract on the host (no GPU here): tests/mesh_shade_ref.py, the numpy restatement the kernels are held to, against closed forms
with exact answers; one named case per planted mistake of the restatement (`variant=`), asserted one by one; the header's prototypes against hip.py.

The pixel camera of the interpolation cases: identity pose, focal 32, the principal point on a pixel centre, every depth a power of two - so a vertex
meant for pixel position (u, v) at depth z has x = (u - cx) z / 32, exact in float32, and projects back to (u, v) exactly."""
import itertools

import numpy as np

import abi_header
import mesh_ref as M
import mesh_shade_ref as S

F = np.float32
H, W, FOCAL, PP, NEAR = 8, 10, 32.0, (4.5, 3.5), 0.05
EYE = np.eye(4)

OCTA_V = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=F)
# outward winding: (sx, 0, 0), (0, sy, 0), (0, 0, sz) is counter-clockwise from outside iff sx sy sz > 0
OCTA_F = np.array([[0 if sx > 0 else 1, 2 if sy > 0 else 3, 4 if sz > 0 else 5][::1 if sx * sy * sz > 0 else -1]
                   for sx, sy, sz in itertools.product((1, -1), repeat=3)], dtype=np.int64)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------- normals
def test_octahedron_normals_are_the_axes_exactly():
    n = S.normals(OCTA_V, OCTA_F)
    assert n.dtype == F and same(n, OCTA_V)
    assert np.array_equal(S.normals(OCTA_V, OCTA_F[:, ::-1]), -OCTA_V)        # flipped winding: exactly negated (a zero sum gives +0 either way)


def test_scale_and_face_order_do_not_change_a_bit():
    rng = np.random.default_rng(3)
    v = (OCTA_V + rng.uniform(-0.2, 0.2, OCTA_V.shape)).astype(F)
    n = S.normals(v, OCTA_F)
    assert same(S.normals(v * F(4), OCTA_F), n)                               # sh moves by -4, every q stays
    assert S.shift(v * F(4)) == S.shift(v) - 4
    acc = S.accumulate(v, OCTA_F)
    for k, perm in enumerate(itertools.permutations(range(8))):
        if k % 97 == 0:                                                       # 416 of the 40 320 orders, the identity and far ones among them
            assert np.array_equal(S.accumulate(v, OCTA_F[list(perm)]), acc)
    assert same(S.normals(v, OCTA_F[::-1]), n)
    neg = S.normals(v, OCTA_F[:, ::-1])
    assert same(neg, -n)


def test_vertices_without_a_valid_face_get_zero():
    v = np.concatenate([OCTA_V, np.array([[5, 5, 5], [np.nan, 0, 0], [2, 0, 0], [3, 0, 0]], dtype=F)])
    f = np.concatenate([OCTA_F, np.array([[6, 7, 0], [6, -1, 0], [6, len(v), 1], [0, 8, 9], [6, 6, 8]])])     # NaN, bad indices, collinear, repeated corner
    n = S.normals(v, f)
    assert same(n[:6], OCTA_V) and not n[6:].any()
    assert S.shift(np.full((3, 3), np.nan, dtype=F)) == 0 and S.shift(np.zeros((4, 3), dtype=F)) == 0
    assert not S.normals(np.zeros((4, 3), dtype=F), [[0, 1, 2]]).any()


def test_the_quantised_vectors_stay_below_2_to_the_52():
    for scale in (2.0 ** -20, 1.0, 3.7, 1e6):
        v = (np.random.default_rng(5).uniform(-1, 1, (50, 3)) * scale).astype(F)
        f = np.random.default_rng(6).integers(0, 50, (400, 3))
        S.accumulate(v, f)                                                    # asserts |q| < 2^52 itself
        sh = S.shift(v)
        D = float(np.max(v.max(axis=0).astype(np.float64) - v.min(axis=0).astype(np.float64)))
        assert 2.0 ** ((51 - sh) // 2 - 1) <= D < 2.0 ** ((51 - sh) // 2)


def test_sqrt_heron_is_within_one_ulp():
    rng = np.random.default_rng(7)
    x = np.concatenate([rng.uniform(0.25, 3, 200000), 2.0 ** rng.integers(-300, 300, 1000) * rng.uniform(1, 2, 1000), [1.0, 4.0, 2.0 ** 100, 2.0 ** -101, 0.5, 3.0]])
    got, want = S.sqrt_heron(x), np.sqrt(x)
    assert (np.abs(got - want) <= np.spacing(want)).all()
    assert S.sqrt_heron(4.0) == 2.0 and S.sqrt_heron(2.0 ** 100) == 2.0 ** 50 and S.sqrt_heron(1.0) == 1.0
    acc = S.accumulate(OCTA_V, OCTA_F)                                        # the values the cases use
    Sx = acc[:, :, 0].astype(np.float64) * 67108864.0 + acc[:, :, 1]
    len2 = (Sx * Sx).sum(axis=1)
    assert (np.abs(S.sqrt_heron(len2) - np.sqrt(len2)) <= np.spacing(np.sqrt(len2))).all()


# ---------------------------------------------------------------- interpolation under the pixel camera
def at(u, v, z):
    return [(u - PP[0]) * z / FOCAL, (v - PP[1]) * z / FOCAL, z]


def cams():
    return M.camera_table([EYE], [[FOCAL, FOCAL]], (H, W), [PP])


def tilted():
    """one face with A > 0 over most of the image with depths 1, 2, 4 and one with A < 0 behind it at depth 8"""
    v = np.array([at(0.25, 0.25, 1.0), at(9.75, 0.5, 2.0), at(1.0, 7.75, 4.0), at(0.0, 0.0, 8.0), at(0.0, 8.0, 8.0), at(10.0, 0.0, 8.0)], dtype=F)
    return v, np.array([[0, 1, 2], [3, 4, 5]], dtype=np.int64)                 # the second has A < 0 as listed: corners 1 and 2 are exchanged


def rendered(v, f):
    return M.render(v, f, [EYE], [[FOCAL, FOCAL]], (H, W), pp=[PP], near=NEAR)


def test_the_camera_z_of_the_vertices_interpolates_to_the_depth():
    v, f = tilted()
    r = rendered(v, f)
    assert set(np.unique(r['face'])) == {-1, 0, 1} and (r['face'] == 0).sum() > 10
    got = S.interp(r['face'], v, f, cams(), NEAR, attr=v[:, 2:3].copy(), fill=0.0)
    assert same(got['attr'][..., 0], r['depth']) and np.array_equal(got['hit'], r['face'] >= 0)


def test_a_power_of_two_constant_comes_back_unchanged_and_a_miss_gets_the_fill():
    v, f = tilted()
    r = rendered(v, f)
    got = S.interp(r['face'], v, f, cams(), NEAR, attr=np.full((len(v), 2), 0.25, dtype=F), fill=-1.0)
    hit = r['face'] >= 0
    assert (got['attr'][hit] == F(0.25)).all() and (got['attr'][~hit] == F(-1)).all() and hit.any() and (~hit).any()


def test_fronto_parallel_shade_is_one_at_the_principal_point():
    v = np.array([at(4.0, 3.0, 2.0), at(4.0, 3.0, 2.0), at(4.0, 3.0, 2.0)], dtype=F)
    v[1, 0] += 1                                                              # e1 = (1, 0, 0), e2 = (0, 1, 0): the face vector is (0, 0, 1)
    v[2, 1] += 1
    f = np.array([[0, 1, 2]])
    r = rendered(v, f)
    assert r['face'][0, 3, 4] == 0                                            # the principal point (4.5, 3.5) is the centre of pixel (3, 4)
    for faces in (f, f[:, ::-1]):                                             # two-sided
        shade = S.interp(r['face'], v, faces, cams(), NEAR, shade_mode=1)['shade']
        assert shade[0, 3, 4] == F(1) and (shade[r['face'] < 0] == 0).all() and (shade[r['face'] == 0] <= 1).all()
        assert (shade[r['face'] == 0] < 1).sum() == (r['face'] == 0).sum() - 1


def test_a_normal_at_right_angles_to_the_ray_gives_shade_zero():
    """edge-on: the ray of a rendered pixel always crosses its face's plane, so the flat shade of a hit is never 0; the case gives the vertices normals
    along x and looks down the column j + 0.5 = cx, where every ray has d0 = 0"""
    v, f = tilted()
    r = rendered(v, f)
    n = np.tile(np.array([[1, 0, 0]], dtype=F), (len(v), 1))
    shade = S.interp(r['face'], v, f, cams(), NEAR, shade_mode=2, normals=n)['shade']
    col = r['face'][0, :, 4] >= 0
    assert col.sum() >= 4 and (shade[0, :, 4][col] == 0).all() and (shade[0, :, 5][r['face'][0, :, 5] >= 0] > 0).all()


def test_a_face_seen_edge_on_is_a_miss_with_shade_zero():
    """the literal case: a face in a plane through the camera centre projects onto a line (A == 0), is never drawn, and a hand-made map that names it
    gets the fill and shade 0 on every pixel, the pixels of that line included"""
    v = np.array([at(2.5, 0.5, 1.0), at(2.5, 0.5, 4.0), at(6.5, 6.5, 2.0), at(0.0, 0.0, 2.0), at(9.0, 1.0, 2.0), at(1.0, 7.0, 2.0)], dtype=F)
    v[1] = v[0] * F(4)                                                        # the same ray: the plane of face 0 holds the camera centre
    f = np.array([[0, 1, 2], [3, 4, 5]])
    s = M.setup(v, f, cams()[0], H, W, NEAR)
    assert list(s['usable']) == [True, True] and list(s['ok']) == [False, True] and s['A'][0] == 0
    face = np.zeros((1, H, W), dtype=np.int64)
    for mode, n in ((1, None), (2, np.tile(np.array([[0, 0, 1]], dtype=F), (6, 1)))):
        got = S.interp(face, v, f, cams(), NEAR, attr=np.ones((6, 1), dtype=F), fill=-1.0, shade_mode=mode, normals=n)
        assert not got['hit'].any() and (got['shade'] == 0).all() and (got['attr'] == F(-1)).all()
    assert (rendered(v, f)['face'] != 0).all() and S.interp(np.ones((1, H, W), dtype=np.int64), v, f, cams(), NEAR, shade_mode=1)['hit'].any()


# ---------------------------------------------------------------- one named case per planted mistake
def test_variants_are_the_listed_ones():
    assert S.VARIANTS == ('no_swap', 'assoc', 'affine', 'trunc', 'unit', 'heron5', 'no_coverage')


def test_planted_no_swap():
    v, f = tilted()
    r = rendered(v, f)
    attr = np.array([[0], [0], [0], [1], [2], [4]], dtype=F)                  # three distinct rows on the clockwise face
    good, bad = (S.interp(r['face'], v, f, cams(), NEAR, attr=attr, variant=x)['attr'] for x in (None, 'no_swap'))
    back, front = r['face'] == 1, r['face'] == 0
    assert back.sum() >= 4 and not same(good[back], bad[back]) and same(good[front], bad[front])


def test_planted_assoc():
    """the two associations differ by an ulp of the fp64 sum, 29 bits below fp32: the case is a face with generic depths and three attribute values whose
    weighted sum all but cancels at pixel (3, 3) (a1 = -b0 / b1 and a2 = the remainder, from the pixel's weights b), so that the ulp is what is left"""
    v = np.array([at(0.3, 0.2, 1.3), at(9.6, 0.7, 2.7), at(1.1, 7.9, 3.9)], dtype=F)
    f = np.array([[0, 1, 2]])
    r = rendered(v, f)
    assert r['face'][0, 3, 3] == 0
    attr = np.array([[1.0], [float.fromhex('-0x1.e6831cp+0')], [float.fromhex('0x1.f67a74p-27')]], dtype=F)
    good, bad = (S.interp(r['face'], v, f, cams(), NEAR, attr=attr, variant=x)['attr'] for x in (None, 'assoc'))
    assert abs(good[0, 3, 3, 0]) < 1e-7 and good[0, 3, 3, 0] != bad[0, 3, 3, 0]


def test_planted_affine():
    v, f = tilted()
    r = rendered(v, f)
    good, bad = (S.interp(r['face'], v, f, cams(), NEAR, attr=v[:, 2:3].copy(), variant=x)['attr'][..., 0] for x in (None, 'affine'))
    front = r['face'] == 0
    assert same(good, r['depth']) and (bad[front] >= good[front]).all() and (bad[front] > good[front]).sum() > front.sum() // 2      # the affine mean overshoots


def test_planted_trunc():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 0.75, 0]], dtype=F)               # the face vector (0, 0, -0.75) with the winding below: q < 0, lo != 0
    f = np.array([[0, 2, 1]])
    acc = S.accumulate(v, f)
    q = acc[0, 2, 0] * 2 ** 26 + acc[0, 2, 1]
    assert q < 0 and acc[0, 2, 1] == 0                                        # 0.75 2^sh is a multiple of 2^26 here: make lo count
    v[1, 0], v[2, 1] = F(1) + F(2.0 ** -23), F(0.75) + F(2.0 ** -23)
    good, bad = S.accumulate(v, f), S.accumulate(v, f, variant='trunc')
    assert good[0, 2, 1] != 0 and good[0, 2, 0] == bad[0, 2, 0] - 1 and np.array_equal(good[:, :, 1], bad[:, :, 1])
    v2 = np.concatenate([v, np.array([[0, 0, 1]], dtype=F)])                  # with a second face the direction itself moves
    f2 = np.array([[0, 2, 1], [0, 1, 3]])
    assert not same(S.normals(v2, f2), S.normals(v2, f2, variant='trunc'))


def test_planted_unit():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 4]], dtype=F)       # at vertex 0: a face of area 1/2 with normal +z, one of area 2 with normal +y
    f = np.array([[0, 1, 2], [0, 3, 1]])
    good, bad = S.normals(v, f), S.normals(v, f, variant='unit')
    assert good[0, 1] > good[0, 2] > 0 and bad[0, 1] == bad[0, 2] and not same(good, bad)


def test_planted_heron5():
    """From s = 1 on r in [0.5, 2) the error after k steps is at most 4.1e-1, 8.6e-2, 2.5e-3, 2.1e-6, 1.6e-12, 9e-25 (largest as r -> 2): the fifth step
    lands on the sixth's value unless r / s4 falls within about 1e-8 ulp of a rounding midpoint, so random sampling does not find a case (0 of 10^6
    here, 0 of 10^8 when the contract was written).  The two named arguments were found by looking for exactly that just below r = 2; at both the
    sixth step moves the result by one ulp, and a seventh changes nothing more."""
    for h, five, six in (('0x1.fffffebce56bap+0', '0x1.6a09e5f5b7b7ap+0', '0x1.6a09e5f5b7b79p+0'), ('0x1.fffffe17e224dp+0', '0x1.6a09e5bb60769p+0', '0x1.6a09e5bb60768p+0')):
        r = float.fromhex(h)
        assert float(S.sqrt_heron(r, 5)).hex() == five and float(S.sqrt_heron(r, 6)).hex() == six == float(S.sqrt_heron(r, 7)).hex()
        assert abs(float(S.sqrt_heron(r)) - np.sqrt(r)) <= np.spacing(np.sqrt(r))
        x = r * 4.0 ** 7                                                      # through the scaling by an even power of two
        assert S.sqrt_heron(x, 5) != S.sqrt_heron(x, 6) == S.sqrt_heron(r) * 2.0 ** 7
    x = np.random.default_rng(13).uniform(0.5, 2, 1 << 20)
    four, five, six = (S.sqrt_heron(x, k) for k in (4, 5, 6))
    assert (four != six).mean() > 0.4 and not (five != six).any()


def test_planted_no_coverage():
    v, f = tilted()
    face = np.full((1, H, W), -1, dtype=np.int64)
    face[0, 7, 9] = 0                                                         # the far corner: inside the image, outside face 0
    assert rendered(v, f)['face'][0, 7, 9] != 0
    good, bad = (S.interp(face, v, f, cams(), NEAR, attr=np.ones((len(v), 1), dtype=F), fill=-1.0, variant=x) for x in (None, 'no_coverage'))
    assert good['attr'][0, 7, 9, 0] == F(-1) and not good['hit'].any() and bad['hit'][0, 7, 9] and bad['attr'][0, 7, 9, 0] != F(-1)


# ---------------------------------------------------------------- the ABI
def test_prototypes_agree_with_the_header_and_the_abi_stays_20():
    from panst3r_amd import hip
    assert hip.ABI_VERSION == 20 == abi_header.defines()['PST_ABI_VERSION']
    code = {'int': 'i', 'int64_t': 'l', 'uint64_t': 'u', 'float': 'f', 'double': 'd'}
    protos = {p[0]: p for p in abi_header.prototypes()}
    for name in ('pst_mesh_normals_accumulate', 'pst_mesh_normals_finish', 'pst_mesh_interp'):
        _, ret, params = protos[name]
        assert hip.SIGNATURES[name] == code[ret] + ':' + ''.join('p' if t.endswith('*') else code[t] for t in params), name
    d = abi_header.defines()
    assert (d['PST_MESH_INTERP_MAX_CHANNELS'], d['PST_MESH_NORMALS_MAX_SHIFT']) == (hip.MESH_INTERP_MAX_CHANNELS, hip.MESH_NORMALS_MAX_SHIFT) == (16, 1100)
    assert (d['PST_MESH_SHADE_NONE'], d['PST_MESH_SHADE_FLAT'], d['PST_MESH_SHADE_SMOOTH']) == (hip.MESH_SHADE_NONE, hip.MESH_SHADE_FLAT, hip.MESH_SHADE_SMOOTH)


def test_the_host_shift_is_the_restatement_s():
    from panst3r_amd.engine.shade import normals_shift
    for scale in (2.0 ** -20, 1.0, 3.7, 1e6):
        v = (np.random.default_rng(5).uniform(-1, 1, (50, 3)) * scale).astype(F)
        assert normals_shift(v.min(axis=0).tolist(), v.max(axis=0).tolist()) == S.shift(v)
    assert normals_shift([np.inf] * 3, [-np.inf] * 3) == 0 and normals_shift([1.0, np.inf, 2.0], [1.0, -np.inf, 2.0]) == 0
