"""ctypes binding of libpanst3r_hip.so (C ABI in include/panst3r_hip.h) for torch device tensors.

PyTorch is plumbing here: it owns the HBM buffers and the HIP stream; every op below passes raw device pointers,
sizes and `torch.cuda.current_stream().cuda_stream` across the C ABI.  There is NO fallback: if the library is
missing or an argument is rejected the op raises (RuntimeError), it never silently computes with torch.

The library sees addresses and a few integers, so the wrapper is the only bounds check of a call.  Every entry point takes each address from
`_Operands`, where the argument goes: a tensor on the GPU, on the device of the call's other operands, of the header's dtype, contiguous - or
(`rows`) a row view at its leading dimension - holding the elements the header states: exactly, or at least (`ge`, `rows`) for a capacity.
A failure is a RuntimeError naming the wrapper, the operand, what was expected and what was found; none is an `assert`, so `python -O` checks the
same.  The GEMM / attention builders name tensor, dtype and device the same way (`any`); the library checks their bounds itself.
"""
import ctypes as C
import math
import os
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('PST_LIB') or os.path.join(_HERE, 'lib', 'libpanst3r_hip.so')      # PST_LIB: A/B builds of the same ABI (measurement)
ABI_VERSION = 20
STATS_BLOCKS = 128        # PST_STATS_BLOCKS
_lib = None

i32, i64, f32, vp = C.c_int32, C.c_int64, C.c_float, C.c_void_p


class GemmParams(C.Structure):
    _fields_ = [('A', vp), ('lda', i64), ('W', vp), ('ldw', i64), ('C', vp), ('ldc', i64),
                ('M', i32), ('N', i32), ('K', i32),
                ('bias', vp), ('gamma', vp), ('res', vp), ('ldr', i64), ('res_mod', i32),
                ('act', i32), ('out_fp32', i32), ('trans_out', i32),
                ('grp_in', i32), ('grp_out', i32), ('grp_off', i32),
                ('ps_p', i32), ('ps_c', i32), ('ps_h', i32), ('ps_w', i32),
                ('conv_c', i32), ('conv_h', i32), ('conv_w', i32), ('zeros', vp), ('rope_pos', vp), ('rope_cs', vp), ('rope_hd', i32), ('rope_npos', i32), ('res_bf16', i32), ('kernel', i32),
                ('batch', i32), ('a_bs', i64), ('w_bs', i64), ('c_bs', i64), ('bias_bs', i64), ('dtype16', i32),
                ('xcopy', vp), ('ldxc', i64), ('stats_out', vp), ('stats_ld', i32), ('ln_stats', vp), ('ln_groups', i32), ('ln_colsum', vp), ('ln_eps', f32), ('x3_block', i32)]


class AttnParams(C.Structure):
    _fields_ = [('Q', vp), ('q_bs', i64), ('q_hs', i64), ('q_rs', i64),
                ('K', vp), ('k_bs', i64), ('k_hs', i64), ('k_rs', i64),
                ('Vt', vp), ('v_bs', i64), ('v_hs', i64), ('v_ds', i64),
                ('O', vp), ('o_bs', i64), ('o_hs', i64), ('o_rs', i64),
                ('mask', vp), ('m_bs', i64), ('m_rs', i64),
                ('B', i32), ('H', i32), ('Nq', i32), ('Nk', i32), ('hd', i32),
                ('scale', f32), ('zeros', vp), ('nsplit', i32), ('ws', vp), ('ws_bytes', i64), ('dtype16', i32), ('prescaled', i32)]


class CloudView(C.Structure):
    _fields_ = [('conf', vp), ('pts3d', vp), ('pts3d_local', vp), ('img', vp), ('pan', vp), ('offset', i64), ('npix', i32), ('first_wg', i32), ('c2w', f32 * 12)]


# The C prototypes, one entry per exported function: 'return:arguments' in the type codes of _CODES; tests/test_abi.py checks every entry against the
# header, and lib() declares them, so a call site passes plain Python numbers and ctypes converts (or refuses) them by the prototype.  The two parameter
# structs the host fills are declared as pointers to them: only that struct is accepted, by reference.  Every other pointer - device memory (the
# pst_cloud_view table included) and the stream - is an address: `_Operands` / `_stream` give plain ints or None.
_CODES = {'i': C.c_int, 'l': C.c_int64, 'u': C.c_uint64, 'f': C.c_float, 'd': C.c_double, 'p': vp, 's': C.c_char_p,
          'G': C.POINTER(GemmParams), 'A': C.POINTER(AttnParams)}
SIGNATURES = {
    'pst_abi_version': 'i:', 'pst_last_error': 's:', 'pst_gemm': 'i:Gp', 'pst_gemm_variant': 's:G', 'pst_gemm_pair': 'i:GGp', 'pst_gemm_pair_variant': 's:GG',
    'pst_tune': 'i:ii', 'pst_mask_head_supported': 'i:iii', 'pst_mask_head': 'i:plplpliiiiip', 'pst_attn_workspace_bytes': 'l:iiiii', 'pst_attn_fwd': 'i:Ap',
    'pst_attn_variant': 's:A', 'pst_attn_pair': 'i:AAp', 'pst_attn_pair_variant': 's:AA', 'pst_layernorm': 'i:pliplippiifiiip',
    'pst_layernorm_add': 'i:pliplplippiifiiip', 'pst_token_embed': 'i:piipipiiplpp', 'pst_rowstats': 'i:pliplpiiiip',
    'pst_layernorm_add_batch': 'i:pliplplippiifiiiilllp', 'pst_split3': 'i:plpliiip', 'pst_split_operand': 'i:plpliiiiip', 'pst_split2': 'i:plppliiiip',
    'pst_transpose_f32': 'i:plpliip', 'pst_rope2d_split': 'i:plppppliiiip', 'pst_attn_x3': 'i:Apppilp', 'pst_attn_x3_variant': 's:A',
    'pst_rope2d': 'i:plppiiiip', 'pst_patchify': 'i:ppliiiiiip', 'pst_dino_preprocess': 'i:ppiiiiip', 'pst_image_prepare': 'i:piipiiiiiip',
    'pst_patch_rows': 'i:pplpliiiiiiip', 'pst_add_cast': 'i:plipliipliiip', 'pst_l2norm_rows': 'i:plpliifip', 'pst_mean4': 'i:ppiiiiip',
    'pst_resize_bilinear': 'i:ppiiiiiiip', 'pst_attn_mask_from_logits': 'i:plpliip', 'pst_loftup_guidance_gn': 'i:ppppfpppliiiiipp',
    'pst_loftup_minmax': 'i:ppiiip', 'pst_minmax_merge': 'i:pppip', 'pst_groupnorm_stats': 'i:plipiiiip', 'pst_groupnorm_apply': 'i:plippppliiiifiip',
    'pst_loftup_lr_pe': 'i:ppliiiiip', 'pst_pp_scores': 'i:piiffpppp', 'pst_pp_scores_softmax': 'i:piifpppp', 'pst_pp_sigmoid': 'i:pppiip',
    'pst_pp_argmax': 'i:pppiiiiifppppp', 'pst_pp_argmax_logits': 'i:pppiiiiifppppp', 'pst_pp_select': 'i:pppidppp', 'pst_pp_finalize': 'i:pppiffppp',
    'pst_qubo_upsample': 'i:ppiiiiip', 'pst_qubo_workspace_floats': 'l:il', 'pst_qubo_overlap': 'i:pilppp', 'pst_qubo_argmax': 'i:ppilppp',
    'pst_pointmap_activate': 'i:pppplip', 'pst_focal_weiszfeld': 'i:pppiiiip', 'pst_rigid_moments': 'i:ppppiifp', 'pst_retrieval_select': 'i:plppiiiplpp',
    'pst_retrieval_assign': 'i:plplpiiiiippppip', 'pst_retrieval_aggregate': 'i:plplpppiippp', 'pst_retrieval_scores': 'i:ppppppiiiiffpp',
    'pst_cloud_count': 'i:piifpp', 'pst_cloud_scan': 'i:pipp', 'pst_cloud_compact': 'i:piifppiffppppppp', 'pst_cloud_segment_median': 'i:ppplpiippppppp',
    'pst_qubo_anneal_max_n': 'i:', 'pst_qubo_anneal': 'i:piiifffuppppp',
    'pst_voxel_insert': 'i:plfplpppip', 'pst_voxel_count': 'i:pplpp', 'pst_voxel_rank': 'i:pplpppp', 'pst_voxel_accumulate': 'i:ppplfpppipppplppip',
    'pst_voxel_vote': 'i:pplpp', 'pst_voxel_emit': 'i:pppplfdppppiffppppppp',
    'pst_render_max_radius': 'i:', 'pst_render_splat': 'i:plpiiifiipip', 'pst_render_resolve': 'i:pllppppppppp',
    'pst_consist_depth': 'i:ppiilfipp', 'pst_consist_count': 'i:pppiilfippppp',
    'pst_tsdf_insert': 'i:pliplpppp', 'pst_tsdf_nodes': 'i:pliplplppppp', 'pst_tsdf_integrate': 'i:plfipppipppp', 'pst_tsdf_cells': 'i:plplpppipppp',
    'pst_tsdf_vertices': 'i:plplpppippppldppppppp', 'pst_tsdf_face_count': 'i:plplpppippppp', 'pst_tsdf_face_emit': 'i:plplppppppppppp',
    'pst_mesh_lane_pixels': 'i:', 'pst_mesh_raster': 'i:plplpiiiffppplip', 'pst_mesh_resolve': 'i:piiiplplpfpppppp', 'pst_mesh_area_count': 'i:pilpiipp',
    'pst_mesh_area_apply': 'i:pilpiipipp',
    'pst_mesh_normals_accumulate': 'i:plplipp', 'pst_mesh_normals_finish': 'i:plpp', 'pst_mesh_interp': 'i:piiiplplpfpifpippp',
    'pst_pq_count': 'i:pplpipipiiipip', 'pst_pq_match': 'i:piiipppppppp',
    'pst_vcc_cells': 'i:ppplfpp', 'pst_vcc_build': 'i:pplpplppp', 'pst_vcc_link': 'i:pplpplippp', 'pst_vcc_flatten': 'i:ppplppppppip', 'pst_vcc_count': 'i:plpp',
    'pst_vcc_rank': 'i:pplpppppppppppppp', 'pst_vcc_votes': 'i:pppplppliipplpp', 'pst_vcc_apply': 'i:pppplippiffpppp',
    'pst_surface_rows': 'i:pllpp', 'pst_surface_count': 'i:ppiipfpp', 'pst_surface_emit': 'i:ppiipfpppppp', 'pst_surface_link': 'i:pllpppp',
    'pst_surface_components': 'i:pllppppp', 'pst_surface_keep_count': 'i:pplipp', 'pst_surface_keep_emit': 'i:ppppplippppp',
    'pst_simplify_used': 'i:pllppp', 'pst_simplify_mask': 'i:pplppp', 'pst_simplify_remap': 'i:pllpliplpppip', 'pst_simplify_count': 'i:pplipp',
    'pst_simplify_emit': 'i:pppppplllipppppp',
    'pst_mesh_sample_count': 'i:plplfipppp', 'pst_mesh_sample_emit': 'i:plplpllppppppp',
    'pst_nn_insert': 'i:plfplpppp', 'pst_nn_scatter': 'i:plpppppp', 'pst_nn_query': 'i:plplffplpppipppp',
    'pst_icp_chunk': 'i:', 'pst_icp_step': 'i:plffffffffffffplffplpppipppppp',
    'pst_meshdist_count': 'i:plplfpppp', 'pst_meshdist_insert': 'i:plplfplplpppp', 'pst_meshdist_scatter': 'i:ppllpppppp',
    'pst_meshdist_query': 'i:plplplffplppplippppp',
    'pst_plane_icp_step': 'i:plfffffffffffffffplplffplppplipppppp',
    'pst_depth_median': 'i:ppiiifffpppppp', 'pst_depth_moments': 'i:ppiipifffppp', 'pst_depth_errors': 'i:ppiipifffpiddddppp',
}
EXPORTS = list(SIGNATURES)


def lib():
    """Load the shared library (once) and declare every prototype of SIGNATURES on it.  Raises if it has not been built -- there is no CPU fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError('libpanst3r_hip.so not found at %s -- run `python -m panst3r_amd.build` (hipcc, gfx950). '
                           'The HIP path has no fallback.' % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    for name, sig in SIGNATURES.items():
        ret, args = sig.split(':')
        fn = getattr(L, name)          # AttributeError if a declared symbol is missing
        fn.restype, fn.argtypes = _CODES[ret], [_CODES[c] for c in args]
    if L.pst_abi_version() != ABI_VERSION:
        raise RuntimeError('libpanst3r_hip.so ABI %d != expected %d; rebuild' % (L.pst_abi_version(), ABI_VERSION))
    _lib = L
    return L


TUNE_PAIR, TUNE_PAIR_RES, TUNE_PAIR_ATTN, TUNE_DEEP_RING, TUNE_ATTN_XCD, TUNE_CUS = 4, 5, 7, 8, 9, 10          # (3, 6 and 11 were knobs of retired experiments: never reused)


def tune(knob, value):
    """pst_tune: set a dispatch tuning knob (measurement tools / tests), returns the previous value"""
    return int(lib().pst_tune(int(knob), int(value)))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _call(what, *args):
    """one launch of the entry point `what` on torch's current stream (every launching entry point takes the stream last); a refusal raises with the
    library's message.  Scalars go in as plain Python numbers: the declared prototype converts them, and refuses what does not fit its type."""
    rc = getattr(lib(), what)(*args, _stream())
    if rc != 0:
        raise RuntimeError('%s failed (%d): %s' % (what, rc, lib().pst_last_error().decode()))


H16 = (torch.bfloat16, torch.float16)        # the two 16-bit storage formats (amp='bf16' / amp='fp16'); all 16-bit operands of a call share one
FMT = H16 + (torch.float32,)                 # ... and fp32 operands: the reference's amp=False mode (gemm_f32 / attn_f32, the precision path)
_TC = {torch.bfloat16: 0, torch.float32: 1, torch.float16: 2}     # element type codes of the C ABI (PST_BF16 / PST_F32 / PST_F16)


def _tc(t):
    return _TC[t.dtype]


def _same16(*ts):
    """dtype16 code of a call: every 16-bit operand must use the same format."""
    dts = {t.dtype for t in ts if t is not None and t.dtype in H16}
    if len(dts) != 1:
        raise RuntimeError('16-bit operands of one call must share one format, got %s' % sorted(str(d) for d in dts))
    return _TC[dts.pop()]


def _fmt(*ts):
    """operand format code of a call whose operands all share ONE storage format (16-bit or, in the amp=False mode, fp32)"""
    dts = {t.dtype for t in ts if t is not None}
    if len(dts) != 1 or next(iter(dts)) not in FMT:
        raise RuntimeError('the operands of this call must share one of the formats bf16 / f16 / f32, got %s' % sorted(str(d) for d in dts))
    return _TC[dts.pop()]


I32, I64, F32, F64, U8 = torch.int32, torch.int64, torch.float32, torch.float64, torch.uint8


def _check_operand(what, name, t, dtypes, n, at_least=False, optional=False, layout='dense', fill=False):
    """the part of an operand check that asks no device (tests/test_operand_check_host.py runs it on CPU tensors): `t` is a tensor of `dtypes` (one or a
    tuple) that holds `n` elements - at least `n` with at_least - or, for a tuple `n`, has exactly that shape, at least those extents with at_least (-1: any).
    layout 'dense': contiguous; 'any': strides are the caller's business; 'rows': a 2-D view with unit column stride (its leading dimension goes to the library) -
    with at_least its rows must not overlap, and where the kernel fills every row up to the leading dimension (`fill`) rows x ld elements lie in the storage behind
    the first.  None passes only where `optional`.  Raises RuntimeError naming the wrapper `what` and the operand."""
    if t is None and optional:
        return
    if not isinstance(t, torch.Tensor):
        raise RuntimeError('%s: %s must be a torch tensor, got %s' % (what, name, type(t).__name__))
    dt, rowview = t.dtype, layout == 'rows' and at_least
    if dt != dtypes and (not isinstance(dtypes, tuple) or dt not in dtypes):
        raise RuntimeError('%s: %s: unexpected dtype %s (want %s)' % (what, name, dt, dtypes))
    if rowview and t.dim() == 2:                                # the model path's operand, the one check of every eager launch: accepted here, refused below
        (r, c), (ld, unit), (rows, cols) = t.shape, t.stride(), n
        rows, cols = (r if rows < 0 else rows), (c if cols < 0 else cols)
        held = t.untyped_storage().nbytes() // t.element_size() - t.storage_offset() if fill else rows * ld
        if unit == 1 and r >= rows and c >= cols and (ld >= cols or rows <= 1) and held >= rows * ld:
            return
    if isinstance(n, tuple):
        sh = t.shape
        if sh != n and (len(sh) != len(n) or [w for w, s in zip(n, sh) if w >= 0 and (w > s if at_least else w != s)]):
            raise RuntimeError('%s: %s must have the shape %s%s (-1: any), got %s' % (what, name, n, ' or more' if at_least else '', tuple(sh)))
    elif t.numel() != n and not (at_least and t.numel() > n):
        raise RuntimeError('%s: %s must hold %s%d elements, got %d' % (what, name, 'at least ' if at_least else '', n, t.numel()))
    if (layout == 'dense' and not t.is_contiguous()) or (layout == 'rows' and (t.dim() != 2 or t.stride(1) != 1)):
        raise RuntimeError('%s: %s must be %s, got shape %s, strides %s' % (what, name, 'contiguous' if layout == 'dense' else 'a row-major 2-D view', tuple(t.shape), t.stride()))
    if rowview:
        raise RuntimeError('%s: %s: %d rows of %d columns%s need a leading dimension of no less and %d elements of storage behind the first, got strides %s and %d'
                           % (what, name, rows, cols, ' filled up to it' if fill else '', rows * ld, t.stride(), held))


class _Operands:
    """the operand checks of ONE call of the wrapper `what`.  `b(name, t, dtypes, n)` is written where the address goes and returns t.data_ptr() - or
    None for an absent optional operand - after `_check_operand` and the device tests: a GPU tensor, on the device of the operands before it."""
    __slots__ = ('what', 'device')

    def __init__(self, what):
        self.what, self.device = what, None

    def __call__(self, name, t, dtypes, n, at_least=False, optional=False, layout='dense', fill=False):
        _check_operand(self.what, name, t, dtypes, n, at_least, optional, layout, fill)
        if t is None:
            return None
        if t.get_device() != self.device:
            self._place(name, t)
        return t.data_ptr()

    def _place(self, name, t):                  # the first operand sets the device of the call
        if t.get_device() < 0:                  # -1: not on a GPU
            raise RuntimeError('%s: %s is a %s tensor: the HIP path runs on the GPU only (no CPU fallback)' % (self.what, name, t.device))
        if self.device is not None:
            raise RuntimeError('%s: %s is on %s, the operands before it on GPU %d' % (self.what, name, t.device, self.device))
        self.device = t.get_device()

    def ge(self, name, t, dtypes, n, optional=False):       # a capacity: at least n elements
        return self(name, t, dtypes, n, True, optional)

    def any(self, name, t, dtypes, optional=False):         # a GEMM / attention operand: its strides go to the library, which checks its bounds
        return self(name, t, dtypes, 0, True, optional, 'any')

    def rows(self, name, t, dtypes, rows, cols, fill=False, optional=False):
        """a row view of `rows` x `cols` or more (-1: its own extent) -> (address, leading dimension); (None, 0) for an absent optional operand"""
        return self(name, t, dtypes, (rows, cols), True, optional, 'rows', fill), (0 if t is None else t.stride(0))

    def own(self, name, t, dtypes):                         # a row view whose own shape sizes its call -> (address, leading dimension, rows, columns)
        return self.rows(name, t, dtypes, -1, -1) + tuple(t.shape)

    def sized(self, name, t, dtype, n=0):
        """an operand whose own length (n at the least) sizes its call -> (address, elements)"""
        return self(name, t, dtype, n, True), t.numel()

    def rows3(self, name, t, dtype):
        """an [n, 3] operand that sizes its call -> (address, n): the two consecutive arguments of the entry points"""
        return self(name, t, dtype, (-1, 3)), t.shape[0]

    def require(self, ok, msg, *args):                      # a condition on the sizes of a call that is no single operand's
        if not ok:
            raise RuntimeError('%s: %s' % (self.what, msg % args))


def _wgs(n, wg=1024):       # workgroups of wg items (CLOUD_WG by default) over n
    return (n + wg - 1) // wg


def _select_workspace(slots, device, nan=0, ws=None):       # csrc/radix_select.h's int32 workspace, zeroed (or the caller's ws) -> ws, hist [slots, 2, 256], prefix, rank [slots, 2], nan [slots * nan]
    ws = torch.zeros(slots * (516 + nan), dtype=torch.int32, device=device) if ws is None else ws
    return (ws, *ws.tensor_split([slots * 512, slots * 514, slots * 516]))


class KernelTimer:
    """Optional per-launch HIP-event timing of the two MFMA kernels (bench.py roofline leg).  Events are recorded on
    torch's current stream, which is the stream the kernels are launched on."""

    def __init__(self):
        self.records = []          # (kernel name, flops, start event, end event)

    def bracket(self, name, flops, tag=None):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.records.append((name, flops, a, b, tag))
        return a, b

    def by_tag(self):
        """per (kernel, shape tag): launches, ms, TFLOP/s -- for tools/shape_profile.py"""
        torch.cuda.synchronize()
        out = {}
        for name, flops, a, b, tag in self.records:
            d = out.setdefault((name, tag), dict(launches=0, ms=0.0, flops=0.0))
            d['launches'] += 1
            d['ms'] += a.elapsed_time(b)
            d['flops'] += flops
        return out

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, flops, a, b, tag in self.records:
            d = out.setdefault(name, dict(launches=0, ms=0.0, flops=0.0, bytes=0.0))
            d['launches'] += 1
            d['ms'] += a.elapsed_time(b)
            d['flops'] += flops
            if tag and tag[0] == 'bytes':
                d['bytes'] += tag[1]
        return out


TIMER = None      # set to a KernelTimer to time launches

# ---- range telemetry (debug): max |x| of every 16-bit tensor the wrapped launches WRITE, per (stage, producer).  One reduction + one
# host sync per tensor, eager launches only (never inside a graph capture, never on the timed path): `with hip.maxabs_telemetry() as log:` around a call,
# `hip.stage(name)` labels the launches of a section (scene.SceneRunner labels its stages).  f16 overflows at 65504: a row of the log near that value says
# WHICH stage of a checkpoint needs bf16 operands - the after-the-fact finite check only says that something did.
MAXABS = None
_STAGE = ['']
F16_MAX = 65504.0


class _Ctx:
    def __init__(self, enter, leave):
        self._enter, self._leave = enter, leave

    def __enter__(self):
        return self._enter()

    def __exit__(self, *exc):
        self._leave()
        return False


def maxabs_telemetry():
    def enter():
        global MAXABS
        MAXABS = {}
        return MAXABS

    def leave():
        global MAXABS
        MAXABS = None
    return _Ctx(enter, leave)


def stage(name):
    return _Ctx(lambda: _STAGE.append(name), lambda: _STAGE.pop())


def note_maxabs(t, what):
    """record max |t| under (current stage, what) while the telemetry is on; non-finite values are recorded as inf"""
    if MAXABS is None or t is None or not torch.is_tensor(t) or t.dtype not in H16 or t.numel() == 0:
        return
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError('hip.maxabs_telemetry() needs eager launches (it synchronises after every producer)')
    v = float(torch.amax(t.abs()).float())
    if v != v:
        v = float('inf')
    key = (_STAGE[-1], what)
    MAXABS[key] = max(MAXABS.get(key, 0.0), v)


def maxabs_report(log, top=None):
    """[(stage, producer, max |x|, fraction of the f16 range)] sorted by magnitude"""
    rows = sorted(((k[0], k[1], v, v / F16_MAX) for k, v in log.items()), key=lambda r: -r[2])
    return rows[:top] if top else rows


def hbm_timed(name, nbytes):
    """Decorator for the HBM-bound streaming ops: with a KernelTimer installed the launch is bracketed by HIP events on the launch stream
    and recorded with its ALGORITHMIC byte count nbytes(*args) (bench.py reports GB/s per stage against the 8 TB/s HBM peak)."""
    def deco(fn):
        def wrapped(*a, **k):
            return _timed(name, 0.0, ('bytes', float(nbytes(*a, **k))) if TIMER is not None else None, fn, *a, **k)
        wrapped.__name__, wrapped.__doc__ = fn.__name__, fn.__doc__
        return wrapped
    return deco


def _timed(name, flops, tag, fn, *a, **k):
    """fn(*a, **k); with a KernelTimer installed, bracketed by two HIP events on the launch stream and recorded as (name, flops, tag).  `name` may be a
    callable: it is asked only when the launch is timed (the kernel's name costs a call into the library)."""
    if TIMER is None:
        return fn(*a, **k)
    ev = TIMER.bracket(name() if callable(name) else name, flops, tag)
    ev[0].record()
    r = fn(*a, **k)
    ev[1].record()
    return r


def _variant(what, unknown, *params):
    """the name of the kernel the C side dispatches these parameters to (no re-derived rule here); `unknown` for parameters it rejects"""
    name = getattr(lib(), what)(*params)
    return name.decode() if name else unknown

_ZERO = {}


def zeros_page(device):
    z = _ZERO.get(device)
    if z is None:
        z = torch.zeros(256, dtype=torch.uint8, device=device)
        _ZERO[device] = z
    return z


# ----------------------------------------------------------------------------------------------------------- GEMM
ACT = {None: 0, 'none': 0, 'gelu': 1, 'relu': 2, 'gelu_tanh': 3}      # 'gelu_tanh' (ABI 20): fp32 operands only (the SigLIP text tower's MLP)


def _gemm_params(a, w, out, bias=None, gamma=None, res=None, res_mod=0, act=None, trans_out=False, grp=None, ps=None, conv=None,
                 M=None, kernel=0, rope=None, batch=None, xcopy=None, stats_out=None, ln=None, x3_block=None):
    """pst_gemm_params of one hip.gemm call + (flops, shape tag) for the kernel timer.
    out = epi(a @ w.T).  a [M,K] 16-bit (row-major view), w [N,K] 16-bit, out 16-bit / fp32 2-D view (or raw buffer for ps).
    a, w, out (and res) all fp32: the amp=False mode's fp32-input-MFMA GEMM (same epilogues; no fused RoPE, no LayerNorm fold).
    LayerNorm fold (include/panst3r_hip.h): producer side `xcopy` (16-bit copy of an fp32 out) and `stats_out` (fp32 [M, N/64, 2]);
    consumer side `ln` = (stats [M, groups, 2], colsum [N], eps) with `a` the raw rows and `w` / `bias` folded at pack time."""
    b = _Operands('gemm')
    p = GemmParams()
    p.W, p.ldw = b.rows('w', w, FMT, 0, 0)
    N, K = w.shape
    if conv is not None:
        cc, ch, cw = conv
        p.conv_c, p.conv_h, p.conv_w = cc, ch, cw
        p.A, p.lda, Mv = b.any('a', a, FMT), cc, a.numel() // cc
        b.require(K == 9 * cc, 'a 3x3 conv over %d channels needs K = %d, got w %s', cc, 9 * cc, tuple(w.shape))
    else:
        (p.A, p.lda), Mv = b.rows('a', a, FMT, 0, 0), (a.shape[0] if M is None else M)
        b.require(a.shape[1] == K, 'a %s and w %s must share K', tuple(a.shape), tuple(w.shape))
    if ps is not None:
        p.ps_p, p.ps_c, p.ps_h, p.ps_w = ps
        p.C, p.ldc = b.any('out', out, FMT), 0
    else:
        p.C, p.ldc = b.rows('out', out, FMT, 0, 0)
    p.dtype16 = _fmt(a, w) if a.dtype == torch.float32 else _same16(a, w, out, res)       # fp32 operands: C / res must be fp32 too (checked by the C side)
    p.M, p.N, p.K = Mv, N, K
    p.zeros = zeros_page(a.device).data_ptr()
    p.bias, p.gamma = b.any('bias', bias, F32, True), b.any('gamma', gamma, F32, True)
    if res is not None:
        (p.res, p.ldr), p.res_mod = b.rows('res', res, FMT, 0, 0), res_mod
        p.res_bf16 = int(res.dtype in H16)
    if batch is not None:        # (count, a_bs, w_bs, c_bs, bias_bs): `a`, `w`, `out`, `bias` are problem 0 of a strided batch
        p.batch, p.a_bs, p.w_bs, p.c_bs, p.bias_bs = batch
    p.act = ACT[act]
    p.out_fp32 = int(out.dtype == torch.float32)
    if x3_block:                    # split store: the fp32 result as the f16 A-operand rows [hi | hi | lo] of the next 3 x f16 GEMM (pst_gemm_params.x3_block)
        b.require(out.dtype == X3_FMT and out.shape[1] >= 3 * x3_block, 'a split store needs an f16 out of at least 3 x3_block columns, got %s %s', out.dtype, tuple(out.shape))
        p.out_fp32, p.x3_block = 1, int(x3_block)
    p.trans_out = int(trans_out)
    p.kernel = kernel
    if rope is not None:            # (pos int32 [rows,2], table fp32 [npos,16,2]): RoPE-2D fused into the store, hd 64
        p.rope_pos, p.rope_cs, p.rope_hd = b.any('rope pos', rope[0], I32), b.any('rope table', rope[1], F32), 64
        p.rope_npos = int(rope[1].shape[0])
    if grp is not None:
        p.grp_in, p.grp_out, p.grp_off = grp
    if xcopy is not None:
        p.xcopy, p.ldxc = b.rows('xcopy', xcopy, a.dtype, 0, 0)
    if stats_out is not None:
        p.stats_out, p.stats_ld = b('stats_out', stats_out, F32, (-1, -1, 2)), stats_out.shape[1]
    if ln is not None:
        st, cs, eps = ln
        p.ln_stats, p.ln_groups, p.ln_colsum, p.ln_eps = b('ln stats', st, F32, (-1, -1, 2)), K // 64, b.any('ln colsum', cs, F32), float(eps)
        b.require(K % 64 == 0 and st.shape[1] == K // 64, 'LayerNorm fold: the statistics must cover exactly the K = %d columns of a, got %s', K, tuple(st.shape))
    tag = (Mv, N, K, 'f32' if out.dtype == torch.float32 else '16', act or '', 'res' if res is not None else '',
           'grp' if grp is not None else '', 'rope' if rope is not None else '', 'conv' if conv is not None else '', 'ps' if ps is not None else '')
    return p, 2.0 * Mv * N * K * (batch[0] if batch else 1), tag


# ----------------------------------------------------------------------------------------------------------- fp32 operands on 3 x 16-bit MFMA
# fp32 mode (the reference's amp=False, and the stages it runs outside its autocast): X3 = True evaluates every contraction on fp32 operands as three
# 16-bit MFMAs on split operands (x = hi + lo in X3_FMT: 22 mantissa bits in f16, the lo x lo term dropped; include/panst3r_hip.h "fp32-grade
# contractions") - one 16-bit GEMM over a 3 x longer K, attention on (hi, lo) planes; ~1e-6 against float64 at a third of the 16-bit matrix rate.
# X3 = False: the fp32-input-MFMA kernels (gemm_f32.hip / attn_f32.hip: exact fp32 products, 1 / 16 of the 16-bit rate).  Switched by
# model.common.precision (amp=False / 'fp32' -> X3; 'fp32_exact' -> the exact kernels).
X3 = True
X3_FMT = torch.float16
X3H = 4            # PST_X3H: output type code of layernorm / attention - f16 rows [hi | hi | lo] (the split A operand of the next GEMM)


def split_operand(x, side, kpad=None, out=None, fmt=None):
    """fp32 x [rows, K] -> 16-bit [rows, 3 kpad] = [hi | hi | lo] (side 0: a GEMM's A operand) or [hi | lo | hi] (side 1: its W operand); zero beyond K"""
    b = _Operands('split_operand')
    px, ldx, rows, K = b.own('x', x, F32)
    kpad = (K + 63) // 64 * 64 if kpad is None else kpad
    if out is None:
        out = torch.empty(rows, 3 * kpad, dtype=fmt or X3_FMT, device=x.device)
    _call('pst_split_operand', px, ldx, *b.rows('out', out, H16, rows, 3 * kpad), rows, K, kpad, side, _tc(out))
    return out


def split2(x, transpose=False, hi=None, lo=None, fmt=None):
    """fp32 x [rows, K] -> (hi, lo) 16-bit planes of x (or of x^T: [K, rows rounded up to 8])"""
    b = _Operands('split2')
    px, ldx, rows, K = b.own('x', x, F32)
    shape = (K, (rows + 7) // 8 * 8) if transpose else (rows, K)
    if hi is None:
        hi, lo = torch.empty(shape, dtype=fmt or X3_FMT, device=x.device), torch.empty(shape, dtype=fmt or X3_FMT, device=x.device)
    (ph, ldo), (pl, ldl) = b.rows('hi', hi, H16, *shape), b.rows('lo', lo, H16, *shape)
    b.require(ldl == ldo and lo.dtype == hi.dtype, 'hi and lo must share one format and leading dimension, got %s at %d and %s at %d', hi.dtype, ldo, lo.dtype, ldl)
    _call('pst_split2', px, ldx, ph, pl, ldo, rows, K, transpose, _tc(hi))
    return hi, lo


def rope2d_split(x, pos, table, nheads, hd, fmt=None):
    """RoPE-2D of the first nheads*hd columns of the fp32 rows x -> Planes(hi, lo) [rows, nheads*hd] of the rotated values (the q | k operand of attention on
    split operands; x is not modified): rope2d_ + split2 in one pass"""
    b = _Operands('rope2d_split')
    cols = nheads * hd
    (px, ldx), rows = b.rows('x', x, F32, -1, cols), x.shape[0]
    hi = torch.empty(rows, cols, dtype=fmt or X3_FMT, device=x.device)
    lo = torch.empty(rows, cols, dtype=fmt or X3_FMT, device=x.device)
    _call('pst_rope2d_split', px, ldx, b('pos', pos, I32, 2 * rows), b('table', table, F32, (-1, hd // 4, 2)), hi.data_ptr(), lo.data_ptr(), cols, rows, nheads, hd, _tc(hi))
    return Planes(hi, lo)


def transpose_f32(x, out):
    """out[c, r] = x[r, c] (fp32; out row-major with leading dimension >= rows)"""
    b = _Operands('transpose_f32')
    px, ldx, rows, cols = b.own('x', x, F32)
    _call('pst_transpose_f32', px, ldx, *b.rows('out', out, F32, cols, rows), rows, cols)
    return out


def _x3_wanted(a, w):
    return a.dtype == torch.float32 and (w.dtype in H16 or (w.dtype == torch.float32 and X3))


def _trans_f32(M, N, out, kw):
    """C^T in fp32 from a 16-bit GEMM (whose kernels store transposed results in 16 bit only): the row-major result goes to scratch and one transpose per
    problem moves it into the caller's (strided) buffer.  Returns (scratch output, kwargs without trans_out, finish())."""
    kw = dict(kw)
    kw['trans_out'] = False
    batch = kw.get('batch')
    cnt = batch[0] if batch else 1
    tmp = torch.empty(cnt, M, N, dtype=torch.float32, device=out.device)
    dst, c_bs = out, (batch[3] if batch else 0)
    if batch:
        kw['batch'] = batch[:3] + (M * N, batch[4])
    ld_out = _Operands('gemm').rows('out', dst, FMT, 0, 0)[1]

    def finish():
        for i in range(cnt):
            o = dst if i == 0 else dst.as_strided((N, M), (ld_out, 1), dst.storage_offset() + i * c_bs)
            transpose_f32(tmp[i], o)
    return tmp[0], kw, finish


def _x3_prepare(a, w, out, kw):
    """One fp32-operand GEMM as a 16-bit GEMM over the 3 x longer K: returns (a3, w3, out', kw', finish).  `w` is a pre-split weight (16-bit [N, 3 Kpad],
    model.common.Packed) or an fp32 matrix split here; `finish()` runs what follows the launch (the transpose of a trans_out result: the 16-bit kernels
    store transposed results in 16 bit only)."""
    kw, b = dict(kw), _Operands('gemm')
    if out.dtype != torch.float32 and not kw.get('x3_block'):
        raise RuntimeError('fp32-operand GEMM: the output must be fp32 (or the split form, x3_block=)')
    conv, batch = kw.get('conv'), kw.get('batch')
    c64 = lambda n: (n + 63) // 64 * 64
    if w.dtype == torch.float32:                 # an fp32 W operand (activations on the W side: mask features, class embeddings; tests): split here
        N = w.shape[0]
        if conv is not None:                     # per tap (the K index of the implicit conv is tap-major)
            cc = conv[0]
            w = split_operand(w.reshape(N * 9, cc), 1, kpad=c64(cc)).reshape(N, 27 * c64(cc))
        elif batch is not None:
            count, a_bs, w_bs, c_bs, bias_bs = batch
            ldw = b.rows('w', w, F32, 0, 0)[1]
            if w_bs != N * ldw:
                raise RuntimeError('fp32-operand GEMM: batched W problems must be stacked row blocks')
            w = split_operand(w.as_strided((count * N, w.shape[1]), (ldw, 1)), 1)
            kw['batch'] = batch = (count, a_bs, N * w.shape[1], c_bs, bias_bs)
            w = w[:N]
        else:
            w = split_operand(w, 1)
    fmt = w.dtype
    if conv is not None:
        cc, ch, cw = conv
        a3 = split_operand(a.reshape(-1, cc), 0, kpad=c64(cc), fmt=fmt)
        b.require(w.shape[1] == 27 * c64(cc), 'a split-packed 3x3 conv weight over %d channels has %d columns, got w %s', cc, 27 * c64(cc), tuple(w.shape))
        kw['conv'] = (3 * c64(cc), ch, cw)
    else:
        kpad = w.shape[1] // 3
        if w.shape[1] != 3 * kpad or kpad % 64 or a.shape[1] > kpad:
            raise RuntimeError('fp32-operand GEMM: a 16-bit W next to an fp32 A must be a split-packed weight [N, 3 Kpad] with Kpad >= K (A %s, W %s)'
                               % (tuple(a.shape), tuple(w.shape)))
        rows = a.shape[0] if kw.get('M') is None else kw['M']
        src = a[:rows]
        if batch is not None:
            count, a_bs, w_bs, c_bs, bias_bs = batch
            lda = b.rows('a', a, F32, 0, 0)[1]
            if a_bs != rows * lda:
                raise RuntimeError('fp32-operand GEMM: batched A problems must be stacked row blocks')
            src = a.as_strided((count * rows, a.shape[1]), (lda, 1))
            kw['batch'] = batch = (count, rows * 3 * kpad, w_bs, c_bs, bias_bs)
            kw['M'] = rows                       # rows of ONE problem (a3 stacks all of them)
        a3 = split_operand(src, 0, kpad=kpad, fmt=fmt)
    finish = None
    if kw.get('trans_out'):
        out, kw, finish = _trans_f32(a3.shape[0] // (batch[0] if batch else 1), w.shape[0], out, kw)
    return a3, w, out, kw, finish


def gemm(a, w, out, **kw):
    """out = epi(a @ w.T): see _gemm_params for the arguments.  fp32 `a` with a pre-split 16-bit `w` (or, under X3, an fp32 `w`): the 3 x 16-bit
    evaluation (_x3_prepare)."""
    if _x3_wanted(a, w):
        a3, w3, o3, kw3, finish = _x3_prepare(a, w, out, kw)
        gemm(a3, w3, o3, **kw3)
        if finish is not None:
            finish()
        return out
    if kw.get('trans_out') and out.dtype == torch.float32 and a.dtype in H16:       # split operands prepared by the producer (LayerNorm PST_X3H), fp32 C^T wanted
        o3, kw3, finish = _trans_f32(a.shape[0] if kw.get('M') is None else kw['M'], w.shape[0], out, kw)
        gemm(a, w, o3, **kw3)
        finish()
        return out
    p, flops, tag = _gemm_params(a, w, out, **kw)
    _timed(lambda: _variant('pst_gemm_variant', 'gemm?', p), flops, tag, _call, 'pst_gemm', p)
    if MAXABS is not None and TIMER is None:
        _note_gemm(out, kw, tag)
    return out


def _note_gemm(out, kw, tag):
    M, N = int(tag[0]), int(tag[1])
    what = 'gemm N=%d K=%s%s' % (N, tag[2], (' ' + kw['act']) if kw.get('act') else '')
    if kw.get('ps') or kw.get('grp') or kw.get('batch') or kw.get('conv'):      # remapped / batched stores: the written region is not a corner of `out`
        return
    # only the region the launch wrote (pad rows / columns of a larger buffer hold whatever was there)
    note_maxabs(out[:N, :M] if kw.get('trans_out') else out[:M, :N], what + ' out')
    xc = kw.get('xcopy')
    note_maxabs(None if xc is None else xc[:M, :N], what + ' 16-bit copy of the residual stream')


def gemm_pair(first, second):
    """Two independent GEMMs, each (a, w, out, kwargs), through pst_gemm_pair: ONE launch when both are small-M problems of the 64 x 64-tile kernel
    (`first` row-major, `second` trans_out: the q|k and V^T projections of the memory build) or two big problems of the same persistent-kernel class
    whose tile lists fill the chip better side by side (the same layer of two independent ViTs), else two launches; same bits either way."""
    (a1, w1, o1, k1), (a2, w2, o2, k2) = first, second
    t32 = lambda a, o, k: k.get('trans_out') and o.dtype == torch.float32 and a.dtype in H16
    if t32(a1, o1, k1) or t32(a2, o2, k2):           # fp32 C^T from split operands: no fused form, two launches
        gemm(a1, w1, o1, **k1)
        gemm(a2, w2, o2, **k2)
        return o1, o2
    if _x3_wanted(a1, w1) or _x3_wanted(a2, w2):
        fin = []
        if _x3_wanted(a1, w1):
            a1, w1, o1x, k1, f = _x3_prepare(a1, w1, o1, k1)
            fin.append(f)
        else:
            o1x = o1
        if _x3_wanted(a2, w2):
            a2, w2, o2x, k2, f = _x3_prepare(a2, w2, o2, k2)
            fin.append(f)
        else:
            o2x = o2
        gemm_pair((a1, w1, o1x, k1), (a2, w2, o2x, k2))
        for f in fin:
            if f is not None:
                f()
        return o1, o2
    p1, f1, t1 = _gemm_params(a1, w1, o1, **k1)
    p2, f2, t2 = _gemm_params(a2, w2, o2, **k2)
    name = _variant('pst_gemm_pair_variant', '', p1, p2) if TIMER is not None else None
    if name == '':                                         # timed and not fused: two attributed launches
        gemm(a1, w1, o1, **k1)
        gemm(a2, w2, o2, **k2)
        return o1, o2
    _timed(name, f1 + f2, t1 + t2, _call, 'pst_gemm_pair', p1, p2)
    if MAXABS is not None and TIMER is None:
        _note_gemm(o1, k1, t1)
        _note_gemm(o2, k2, t2)
    return o1, o2


# ----------------------------------------------------------------------------------------------------------- attention
def mask_head_supported(Q, P, C):
    return bool(lib().pst_mask_head_supported(Q, P, C))


def mask_head(embed, feats, out):
    """pred_masks of ALL views of a shape group in one launch (pst_mask_head): embed 16-bit [Q, C], feats 16-bit [n, P, C] (or [n, Hm, Wm, C]),
    out fp32 [n, Q, P] (or [n, Q, Hm, Wm]); bit-identical to n calls of gemm(embed, feats[i], out[i])."""
    b = _Operands('mask_head')
    pe, lde, Q, C = b.own('embed', embed, H16)
    pf = b.ge('feats', feats, H16, 1)
    b.require(feats.dim() >= 2 and feats.shape[-1] == C, 'feats %s must end in the %d channels of embed', tuple(feats.shape), C)
    n = feats.shape[0]
    P = feats.numel() // (n * C)
    _timed('mask_head_kernel', 2.0 * n * Q * P * C, ('bytes', float(n * (C * P * 2 + Q * P * 4))), _call,
           'pst_mask_head', pe, lde, pf, P * C, b('out', out, F32, n * Q * P), Q * P, n, Q, P, C, _same16(embed, feats))
    return out


def auto_nsplit(B, H, Nq, Nk):
    """Key-range splits for few-query / many-key attention (memory build, query decoder): fill ~2 blocks per CU."""
    blocks = ((Nq + 63) // 64) * H * B
    if blocks >= 256 or Nk < 1024:
        return 1
    # long memories (the build's 768 queries x 12 heads against >= 6 144 keys): enough splits that 128-query blocks fill the chip - pst_attn_fwd
    # takes its 128-query variant when blocks x splits >= 256, and every K / V fragment read then feeds two MFMAs (measured, tools/attn_split_bench.py:
    # 11 520 keys 54.1 -> 48.3 us, 24 576 keys 103.4 -> 82.7 us; below 6 144 keys the 64-query blocks with 3 splits stay ahead)
    # round 4 (XCD-contiguous block order, tools/nsplit_bench.py -> profiles/r4_nsplit_bench.txt): two blocks per CU, not three - 7 splits of the build's 72
    # blocks beat 9 - 10 from 5 376 keys on (11 520 keys: 46.1 -> 45.6 us, 9 216: 41.6 -> 39.3, 5 376: 31.0 with 3 splits of 64-query blocks -> 29.6)
    blocks128 = ((Nq + 127) // 128) * H * B
    if Nk >= 5376:
        ns = min(512 // blocks128, Nk // 768, 12) if Nk <= 12288 else min(768 // blocks128, Nk // 1024, 12)        # (beyond 16 keyframes: the round-3 rule, not re-swept)
        if blocks128 * ns >= 256:
            return ns
    return max(1, min(512 // blocks, Nk // 512, 32))


LOG2E = 1.4426950408889634


def attn_workspace_floats(B, H, Nq, Nk, hd, nsplit=None):
    """fp32 elements of split-K workspace `attention` needs for this call (0 when it does not split)."""
    ns = auto_nsplit(B, H, Nq, Nk) if nsplit is None else nsplit
    return ns * B * H * Nq * (hd + 2) if ns > 1 else 0


def _attn_struct(fmt, q, k, vt, out, B, H, Nq, Nk, hd, q_strides, k_strides, v_strides, o_strides, scale, mask, mask_strides, ns, ws, prescaled):
    """pst_attn_params of operands in the format code `fmt`, q / k / vt given as addresses, over `ns` key-range splits (+ the workspace the caller
    must keep alive)"""
    p, b = AttnParams(), _Operands('attention')
    p.dtype16 = fmt
    p.Q, (p.q_bs, p.q_hs, p.q_rs) = q, q_strides
    p.K, (p.k_bs, p.k_hs, p.k_rs) = k, k_strides
    p.Vt, (p.v_bs, p.v_hs, p.v_ds) = vt, v_strides
    p.O, (p.o_bs, p.o_hs, p.o_rs) = out.data_ptr(), o_strides
    if mask is not None:
        p.mask, (p.m_bs, p.m_rs) = b.any('mask', mask, U8), mask_strides
    p.B, p.H, p.Nq, p.Nk, p.hd = B, H, Nq, Nk, hd
    p.scale = float(hd ** -0.5 if scale is None else scale)
    p.prescaled = 1 if prescaled else 0
    p.zeros = zeros_page(out.device).data_ptr()
    if ns > 1:
        n = attn_workspace_floats(B, H, Nq, Nk, hd, ns)
        if ws is None:          # caller-owned workspace preferred (C ABI: the caller owns every buffer); else one from torch's caching allocator
            ws = torch.empty(n, dtype=torch.float32, device=out.device)
        p.nsplit, p.ws, p.ws_bytes = ns, b.ge('ws', ws, F32, n), ws.numel() * 4
    return p, ws


def _attn_params(q, k, vt, out, B, H, Nq, Nk, hd, q_strides, k_strides, v_strides, o_strides, scale=None, mask=None,
                 mask_strides=(0, 0), nsplit=None, ws=None, prescaled=False):
    """pst_attn_params of one hip.attention call (+ the tensors it must keep alive, flops, shape tag)"""
    b = _Operands('attention')
    pq, pk, pv = b.any('q', q, FMT), b.any('k', k, FMT), b.any('vt', vt, FMT)
    b.any('out', out, FMT)
    ns = auto_nsplit(B, H, Nq, Nk) if nsplit is None else nsplit
    if q.dtype == torch.float32 and nsplit is None:
        ns = 1                      # the fp32 kernel does not split the key range
    p, ws = _attn_struct(_fmt(q, k, vt, out), pq, pk, pv, out, B, H, Nq, Nk, hd, q_strides, k_strides, v_strides, o_strides,
                         scale, mask, mask_strides, ns, ws, prescaled)
    return p, ws, 4.0 * B * H * Nq * Nk * hd, (B, H, Nq, Nk, hd)


def attention(q, k, vt, out, B, H, Nq, Nk, hd, q_strides, k_strides, v_strides, o_strides, scale=None, mask=None,
              mask_strides=(0, 0), nsplit=None, ws=None, prescaled=False):
    """Strided flash attention; *_strides = (batch, head, row) in elements (v: batch, head, head-dim row).
    prescaled: q was produced with scale * LOG2E folded in (see `qscale`): softmax in the exp2 domain without a per-score multiply."""
    if (isinstance(q, Planes) or q.dtype == torch.float32) and X3:
        return _attention_x3(q, k, vt, out, B, H, Nq, Nk, hd, q_strides, k_strides, v_strides, o_strides, scale, mask, mask_strides, nsplit, ws, prescaled)
    p, ws, flops, tag = _attn_params(q, k, vt, out, B, H, Nq, Nk, hd, q_strides, k_strides, v_strides, o_strides, scale, mask, mask_strides, nsplit, ws, prescaled)
    _timed(lambda: _variant('pst_attn_variant', 'attn?', p), flops, tag, _call, 'pst_attn_fwd', p)
    if TIMER is None:
        note_maxabs(out, 'attention hd=%d out' % hd)
    return out


def _span(B, H, N, strides, width):
    """[min, max) element offsets (relative to the operand's pointer) an attention operand with (batch, head, row) strides touches"""
    bs, hs, rs = strides
    offs = [b * bs + h * hs + r * rs for b in (0, B - 1) for h in (0, H - 1) for r in (0, N - 1)]
    return min(offs), max(offs) + width


def _attention_x3(q, k, vt, out, B, H, Nq, Nk, hd, q_strides, k_strides, v_strides, o_strides, scale, mask, mask_strides, nsplit, ws, prescaled):
    """attention on fp32 operands as 3 x 16-bit MFMA (pst_attn_x3): the memory spans the call touches are split into (hi, lo) planes once - operands
    that share a buffer (q | k of one projection, both halves of a pair) share the pass - and the kernel reads the planes with the caller's strides."""
    b = _Operands('attention')
    b.any('out', out, (F32, X3_FMT))            # fp32, or (16-bit `out` [rows, 3 x block]) the split A operand of the output projection: PST_X3H
    out_type, out_block = (1, 0) if out.dtype == torch.float32 else (X3H, out.shape[-1] // 3)
    dev = out.device
    spans = []
    for name, t, (lo_, hi_) in (('q', q, _span(B, H, Nq, q_strides, hd)), ('k', k, _span(B, H, Nk, k_strides, hd)),
                                ('vt', vt, _span(B, H, hd, v_strides, (Nk + 7) // 8 * 8))):         # (the kernel reads V^T in 8-key chunks: the last one may reach into the row's pad)
        if isinstance(t, Planes):               # prepared by the caller
            continue
        addr = b.any(name, t, F32)
        # (whole 16-byte groups: a key count that is not a multiple of 4 - DINOv2's 769 - ends inside the pad columns every V^T buffer carries)
        spans.append([addr + 4 * lo_, addr + 4 * ((hi_ + 3) // 4 * 4)])
    merged = []
    for a0, a1 in sorted(spans):
        if merged and a0 <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], a1)
        else:
            merged.append([a0, a1])
    planes = []
    for a0, a1 in merged:
        n = (a1 - a0) // 4
        b.require(a0 % 16 == 0 and n % 4 == 0, 'the operands must be 16-byte aligned with strides that are multiples of 8')
        hi = torch.empty(n, dtype=X3_FMT, device=dev)
        lo = torch.empty(n, dtype=X3_FMT, device=dev)
        _call('pst_split2', a0, n, hi.data_ptr(), lo.data_ptr(), n, 1, n, 0, _TC[X3_FMT])
        planes.append((a0, a1, hi, lo))

    def plane_ptrs(t):
        if isinstance(t, Planes):
            return t.hi.data_ptr(), t.lo.data_ptr()
        addr = t.data_ptr()
        for a0, a1, hi, lo in planes:
            if a0 <= addr < a1:                   # (an operand's own span always contains its pointer: offset 0 is one of the offsets it touches)
                off = (addr - a0) // 2            # fp32 byte offset -> 16-bit byte offset
                return hi.data_ptr() + off, lo.data_ptr() + off
        raise RuntimeError('attention: operand outside the planes')
    (qh, ql), (kh, kl), (vh, vl) = plane_ptrs(q), plane_ptrs(k), plane_ptrs(vt)
    p, ws = _attn_struct(_TC[X3_FMT], qh, kh, vh, out, B, H, Nq, Nk, hd, q_strides, k_strides, v_strides, o_strides, scale, mask, mask_strides,
                         auto_nsplit(B, H, Nq, Nk) if nsplit is None else nsplit, ws, prescaled)
    _timed(lambda: _variant('pst_attn_x3_variant', 'attn_x3?', p), 3 * 4.0 * B * H * Nq * Nk * hd, (B, H, Nq, Nk, hd), _call,
           'pst_attn_x3', p, ql, kl, vl, out_type, out_block)
    return out


def attention_pair(first, second):
    """Two independent attention calls, each (args tuple, kwargs dict) of hip.attention, through pst_attn_pair: ONE launch over both block lists when both
    take the same 128-query kernel variant (the self-attentions of two ViT towers in lock-step), else two launches; same bits either way."""
    (a1, k1), (a2, k2) = first, second
    if (isinstance(a1[0], Planes) or a1[0].dtype == torch.float32) and X3:
        attention(*a1, **k1)
        attention(*a2, **k2)
        return
    p1, w1, f1, t1 = _attn_params(*a1, **k1)
    p2, w2, f2, t2 = _attn_params(*a2, **k2)
    name = _variant('pst_attn_pair_variant', '', p1, p2) if TIMER is not None else None
    if name == '':                                         # timed and not fused: two attributed launches
        attention(*a1, **k1)
        attention(*a2, **k2)
        return
    _timed(name, f1 + f2, t1 + t2, _call, 'pst_attn_pair', p1, p2)
    if TIMER is None:
        note_maxabs(a1[3], 'attention hd=%d out' % a1[8])
        note_maxabs(a2[3], 'attention hd=%d out' % a2[8])


# ----------------------------------------------------------------------------------------------------------- the rest
def _ln_views(b, x, add, out, rows, D, grp, split):
    """the checked row views of a LayerNorm call -> ((x, ldx, type, add, ld_add, out, ldo, type), grp): `x` and `add` hold the remapped last row (the kernel reads
    irow = (row / grp_in) * grp_out + grp_off + row % grp_in), `out` holds `rows` rows - as a split store (PST_X3H) three blocks of ldo / 3 >= D columns"""
    g = grp or (0, 0, 0)
    last = rows - 1
    xrows = max(0, ((last // g[0]) * g[1] + g[2] + last % g[0] if g[0] > 0 else last) + 1)
    px, ldx = b.rows('x', x, FMT, xrows, D)
    pa, lda = b.rows('add', add, F32, xrows, D, optional=True)
    po, ldo = b.rows('out', out, X3_FMT if split else FMT, rows, 3 * D if split else D, fill=split)
    return (px, ldx, _tc(x), pa, lda, po, ldo, X3H if split else _tc(out)), g


def layernorm_batch(x_all, gamma_all, beta_all, out_all, eps, rows=None, grp=None, add=None, split=False):
    """out_all[i] = LN(x_all[i] [+ add]) * gamma_all[i] + beta_all[i] for i < n in ONE launch; x_all [n, R, D], out_all [n, rows, D]
    (split=True: out_all f16 [n, rows, 3 D] = the split A operand rows [hi | hi | lo], PST_X3H)."""
    b = _Operands('layernorm_batch')
    pg = b('gamma_all', gamma_all, F32, (-1, -1))
    pb = b('beta_all', beta_all, F32, tuple(gamma_all.shape))
    px, po = b.any('x_all', x_all, FMT), b.any('out_all', out_all, FMT)
    n, D = x_all.shape[0], gamma_all.shape[1]
    b.require(x_all.dim() == 3 and out_all.dim() == 3 and 0 < n <= min(out_all.shape[0], gamma_all.shape[0]), 'x_all and out_all must be [n, rows, columns] next to '
              'gamma_all / beta_all [n or more, D], got %s, %s and %s', tuple(x_all.shape), tuple(out_all.shape), tuple(gamma_all.shape))
    rows = out_all.shape[1] if rows is None else rows
    v, g = _ln_views(b, x_all[n - 1], add, out_all[n - 1], rows, D, grp, split)      # the last problem: the batch strides keep every one inside the operands
    _call('pst_layernorm_add_batch', px, *v[1:5], po, *v[6:], pg, pb, rows, D, eps, *g, n, x_all.stride(0), out_all.stride(0), D)
    return out_all


@hbm_timed('layernorm', lambda x, gamma, beta, out, eps, rows=None, grp=None, add=None, split=False: (out.shape[0] if rows is None else rows) * gamma.numel() * (x.element_size() + (6 if split else out.element_size()) + (4 if add is not None else 0)))
def layernorm(x, gamma, beta, out, eps, rows=None, grp=None, add=None, split=False):
    """out = LN(x [+ add]); `add`: optional fp32 rows indexed like x (fused residual-style addend).  split=True: `out` f16 [rows, 3 x block] receives the
    result as the split A operand of a 3 x f16 GEMM (rows [hi | hi | lo], PST_X3H) - what split_operand(side 0) would make of the fp32 result."""
    b = _Operands('layernorm')
    pg, D = b.sized('gamma', gamma, F32)
    b.require(add is None or not split, 'a split output takes no addend')
    rows = out.shape[0] if rows is None else rows
    v, g = _ln_views(b, x, add, out, rows, D, grp, split)
    tail = (pg, b('beta', beta, F32, D), rows, D, eps, *g)
    if add is not None:
        _call('pst_layernorm_add', *v, *tail)
    else:
        _call('pst_layernorm', *v[:3], *v[5:], *tail)
        note_maxabs(out[:rows, :D] if MAXABS is not None and not split else None, 'layernorm D=%d out' % D)      # only the region the launch wrote
    return out


@hbm_timed('rowstats', lambda x, xcopy, stats: x.numel() * (x.element_size() + (2 if xcopy is not None else 0)))
def rowstats(x, xcopy, stats):
    """LayerNorm-fold producer outputs for a stream no GEMM wrote: per-row (sum, sumsq) per 64-column group, plus the 16-bit copy of an
    fp32 stream (xcopy=None when x already is the 16-bit stream)."""
    b = _Operands('rowstats')
    px, ldx, rows, D = b.own('x', x, FMT if xcopy is not None else H16)         # (no 16-bit copy: x is the 16-bit stream)
    pc, ldc = b.rows('xcopy', xcopy, H16, rows, D, optional=True)
    ps = b('stats', stats, F32, (-1, -1, 2))
    b.require(stats.shape[0] >= rows and stats.shape[1] * 64 >= D, 'stats must be [%d or more, %d or more, 2], got %s', rows, (D + 63) // 64, tuple(stats.shape))
    _call('pst_rowstats', px, ldx, _tc(x), pc, ldc, ps, stats.shape[1], rows, D, _tc(x if xcopy is None else xcopy))
    if MAXABS is not None and xcopy is not None:
        note_maxabs(xcopy[:rows, :D], 'rowstats D=%d 16-bit copy of the residual stream' % D)
    return xcopy, stats


def split3(x, out):
    """fp32 x [rows, K] -> bf16 out [rows, 3K] = [x_hi | x_hi | x_lo] (operand of a split-precision GEMM, see pack_split3)."""
    b = _Operands('split3')
    px, ldx, rows, K = b.own('x', x, F32)
    _call('pst_split3', px, ldx, *b.rows('out', out, H16, rows, 3 * K), rows, K, _tc(out))
    return out


def pack_split3(weight, dtype=torch.bfloat16):
    """fp32 weight [N, K] -> 16-bit [N, 3K] = [W_hi | W_lo | W_hi] (pack time): with split3(x) one GEMM gives x_hi W_hi + x_hi W_lo + x_lo W_hi."""
    w = weight.detach().float()
    hi = w.to(dtype)
    lo = (w - hi.float()).to(dtype)
    return torch.cat([hi, lo, hi], dim=1).contiguous()


def rope2d_(x, pos, table, nheads, hd):
    """In-place RoPE-2D on the first nheads*hd columns of the row-major bf16 view x; pos int32 [rows,2]."""
    b = _Operands('rope2d_')
    (px, ldx), rows = b.rows('x', x, FMT, -1, nheads * hd), x.shape[0]
    _call('pst_rope2d', px, ldx, b('pos', pos, I32, 2 * rows), b('table', table, F32, (-1, hd // 4, 2)), rows, nheads, hd, _tc(x))
    return x


def rope_table(npos, hd, base=100.0, device='cuda'):
    """fp32 [npos, hd/4, 2] (cos, sin) for RoPE-2D: per half D = hd/2 channels, inv_freq_i = base^(-2i/D)."""
    D = hd // 2
    inv = 1.0 / (base ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    ang = torch.outer(torch.arange(npos, dtype=torch.float32), inv)
    return torch.stack([ang.cos(), ang.sin()], dim=-1).contiguous().to(device)


def patchify(img, out, p):
    b = _Operands('patchify')
    pimg = b('img', img, F32, (-1, -1, -1, -1))
    n, c, h, w = img.shape
    rows = n * (h // p) * (w // p) if p > 0 else 0
    _call('pst_patchify', pimg, *b.rows('out', out, FMT, rows, c * p * p, fill=True), n, c, h, w, p, _tc(out))
    return out


def dino_preprocess(img, out):
    b = _Operands('dino_preprocess')
    pimg = b('img', img, F32, (-1, 3, -1, -1))
    n, _, h, w = img.shape
    _call('pst_dino_preprocess', pimg, b('out', out, F32, (n, 3, -1, -1)), n, h, w, out.shape[-2], out.shape[-1])
    return out


def image_prepare(src_u8, out, resized, crop_origin):
    """decoded uint8 [Hs, Ws, 3] (device) -> fp32 `out` [3, H, W] in [-1, 1]: ImgNorm, antialiased bilinear resize to `resized` = (Hr, Wr),
    crop of out's size at `crop_origin` = (top, left)."""
    b = _Operands('image_prepare')
    src, dst = b('src_u8', src_u8, U8, (-1, -1, 3)), b('out', out, F32, (3, -1, -1))
    (Hs, Ws), (H, W) = src_u8.shape[:2], out.shape[1:]
    Hr, Wr, top, left = int(resized[0]), int(resized[1]), int(crop_origin[0]), int(crop_origin[1])
    b.require(min(Hs, Ws, H, W, Hr, Wr) > 0, 'every size must be positive, got src %d x %d, resized %d x %d, out %d x %d', Hs, Ws, Hr, Wr, H, W)
    b.require(top >= 0 and left >= 0 and top + H <= Hr and left + W <= Wr,
              'the crop must lie inside the resized image %d x %d, got %d x %d at (%d, %d)', Hr, Wr, H, W, top, left)
    _call('pst_image_prepare', src, Hs, Ws, dst, Hr, Wr, top, left, H, W)
    return out


@hbm_timed('patch_rows', lambda img, enc=None, dino=None, **k: img.numel() * 4 + (enc.numel() * 2 if enc is not None else 0) + (dino.numel() * 2 if dino is not None else 0))
def patch_rows(img, enc=None, dino=None, p_enc=16, p_dino=14, dino_transposed=False):
    """fp32 images [n, 3, H, W] -> patch rows of the encoder (`enc` 16-bit [n*T, >= 3 p^2]) and / or DINOv2 (`dino`) in one launch."""
    b = _Operands('patch_rows')
    p_enc, p_dino = int(p_enc), int(p_dino)
    pimg = b('img', img, F32, (-1, 3, -1, -1))
    n, _, H, W = img.shape
    b.require(enc is not None or dino is not None, 'needs enc or dino (or both), got neither')
    b.require(n > 0 and p_enc > 0 and H > 0 and W > 0 and H % p_enc == 0 and W % p_enc == 0,
              'img must hold images whose sides are multiples of p_enc = %d, got %d of %d x %d', p_enc, n, H, W)
    b.require(p_dino > 0 or dino is None, 'p_dino must be positive, got %d', p_dino)
    rows = n * (H // p_enc) * (W // p_enc)
    views = b.rows('enc', enc, FMT, rows, 3 * p_enc * p_enc, True, True) + b.rows('dino', dino, FMT, rows, 3 * p_dino * p_dino, True, True)
    b.require(enc is None or dino is None or enc.dtype == dino.dtype, 'enc and dino must share one of the formats bf16 / f16 / f32, got %s and %s',
              getattr(enc, 'dtype', None), getattr(dino, 'dtype', None))
    _call('pst_patch_rows', pimg, *views, n, H, W, p_enc, p_dino, bool(dino_transposed), _tc(enc if enc is not None else dino))
    return enc, dino


def add_cast(a, out, b=None, b_mod=0):
    c = _Operands('add_cast')
    po, ldo, rows, D = c.own('out', out, FMT)
    _call('pst_add_cast', *c.rows('a', a, FMT, rows, D), _tc(a), *c.rows('b', b, FMT, b_mod if b_mod > 0 else rows, D, optional=True),
          _tc(b) if b is not None else 0, b_mod, po, ldo, _tc(out), rows, D)
    if MAXABS is not None:
        note_maxabs(out[:rows, :D], 'add_cast D=%d out' % D)
    return out


@hbm_timed('token_embed', lambda ids, tok, pos, out, status=None: ids.numel() * (4 + 3 * 4 * tok.shape[1]))
def token_embed(ids, tok, pos, out, status=None):
    """out[b L + l] = tok[ids[b, l]] + pos[l]: ids int32 [B, L], tok fp32 [vocab, D], pos fp32 [npos, D], out fp32 [B L, D] rows (the SigLIP text
    tower's embeddings).  The ids must be in range (the tower checks them on the host); the kernel never reads outside `tok` - an id that is not
    writes a zero row and PST_EINVAL into the optional int32 device scalar `status`."""
    b = _Operands('token_embed')
    pi, pt = b('ids', ids, I32, (-1, -1)), b('tok', tok, F32, (-1, -1))
    (B, L), (vocab, D) = ids.shape, tok.shape
    pp = b('pos', pos, F32, (-1, D))
    po, ldo = b.rows('out', out, F32, B * L, D)
    b.require(out.shape[1] == D, 'out must have the %d columns of tok, got %s', D, tuple(out.shape))
    _call('pst_token_embed', pi, B, L, pt, vocab, pp, pos.shape[0], D, po, ldo, b.ge('status', status, I32, 1, optional=True))
    return out


def l2norm_rows(x, out, eps):
    b = _Operands('l2norm_rows')
    px, ldx, rows, D = b.own('x', x, F32)
    _call('pst_l2norm_rows', px, ldx, *b.rows('out', out, FMT, rows, D), rows, D, eps, _tc(out))
    return out


@hbm_timed('mean4', lambda F, Fm, nimg, Hm, Wm, Cc: Fm.numel() * 2 * 5)
def mean4(F, Fm, nimg, Hm, Wm, Cc):
    b, fmt = _Operands('mean4'), _fmt(F, Fm)
    _call('pst_mean4', b('F', F, FMT, nimg * Hm * Wm * Cc), b('Fm', Fm, FMT, nimg * (Hm // 8) * (Wm // 8) * Cc), nimg, Hm, Wm, Cc, fmt)
    return Fm


def resize_bilinear(F, Fd, nimg, Hs, Ws, Hd, Wd, Cc):
    b, fmt = _Operands('resize_bilinear'), _fmt(F, Fd)
    _call('pst_resize_bilinear', b('F', F, FMT, nimg * Hs * Ws * Cc), b('Fd', Fd, FMT, nimg * Hd * Wd * Cc), nimg, Hs, Ws, Hd, Wd, Cc, fmt)
    return Fd


def attn_mask_from_logits(logits, mask):
    b = _Operands('attn_mask_from_logits')
    pl, ldl, Q, Nk = b.own('logits', logits, F32)
    _call('pst_attn_mask_from_logits', pl, ldl, *b.rows('mask', mask, U8, Q, Nk), Q, Nk)
    return mask


def stats_buffer(nimg, G, device):
    """fp32 statistics buffer for loftup_guidance (G=1) / groupnorm_stats: result [nimg, G, 2] + per-block partials."""
    return torch.empty(nimg * G * 2 * (1 + STATS_BLOCKS), dtype=torch.float32, device=device)


@hbm_timed('loftup_guidance_gn', lambda img, biases, gamma, beta, eps, scratch, stats, out, nf, mm=None: img.numel() * 4 + out.numel() * 2)
def loftup_guidance_gn(img, biases, gamma, beta, eps, scratch, stats, out, nf, mm=None):
    """Fourier guidance features + GroupNorm(1) straight to bf16 `out` [nimg*P, ld] (zero-padded columns); no fp32 feature buffer.
    mm: None = MinMaxScaler per view; else fp32 [nimg, 3, 2] (min, max) to scale with (loftup_minmax / minmax_merge: a scope of several views)."""
    b = _Operands('loftup_guidance_gn')
    pimg = b('img', img, F32, (-1, 3, -1, -1))
    n, _, h, w = img.shape
    P, ch = (h // 2) * (w // 2), 10 * nf + 3
    _call('pst_loftup_guidance_gn', pimg, b('biases', biases, F32, 10 * nf), b.ge('gamma', gamma, F32, ch), b.ge('beta', beta, F32, ch), eps,
          b.ge('scratch', scratch, F32, n * (3 * P + 6)), b.ge('stats', stats, F32, n * 2 * (1 + STATS_BLOCKS)),
          *b.rows('out', out, FMT, n * P, ch, fill=True), n, h, w, nf, _tc(out), b('mm', mm, F32, (n, 3, 2), optional=True))
    return out


def loftup_minmax(img, mm):
    """per (view, channel) (min, max) of the 2x2-mean (= bilinear x0.5) image: img fp32 [n, 3, H, W] -> mm fp32 [n, 3, 2]"""
    b = _Operands('loftup_minmax')
    pimg = b('img', img, F32, (-1, 3, -1, -1))
    n, _, h, w = img.shape
    _call('pst_loftup_minmax', pimg, b('mm', mm, F32, (n, 3, 2)), n, h, w)
    return mm


def minmax_merge(mm, scope, out):
    """out[v] = (min, max) over the views u with scope[u] == scope[v] of mm[u] (the reference's MinMaxScaler over a chunk of views, loftup.py:14-19)"""
    b = _Operands('minmax_merge')
    ps, n = b.sized('scope', scope, I32)
    pm, po = b('mm', mm, F32, (n, 3, 2)), b('out', out, F32, (n, 3, 2))
    b.require(pm != po, 'out of place only: mm and out are the same buffer')
    _call('pst_minmax_merge', pm, ps, po, n)
    return out


@hbm_timed('groupnorm_stats', lambda x, stats, nimg, P, Cc, G: nimg * P * Cc * x.element_size())
def groupnorm_stats(x, stats, nimg, P, Cc, G):
    """(sum, sum of squares) per (view, group) of the pixel-major x [nimg P, Cc] -> stats (stats_buffer: the result [nimg, G, 2], per-block partial sums behind it)"""
    b = _Operands('groupnorm_stats')
    _call('pst_groupnorm_stats', *b.rows('x', x, FMT, nimg * P, Cc), _tc(x), b.ge('stats', stats, F32, nimg * G * 2 * (1 + STATS_BLOCKS)), nimg, P, Cc, G)


@hbm_timed('groupnorm_apply', lambda x, stats, gamma, beta, out, nimg, P, Cc, G, eps, relu, split=False: nimg * P * (Cc * x.element_size() + out.shape[1] * 2))
def groupnorm_apply(x, stats, gamma, beta, out, nimg, P, Cc, G, eps, relu, split=False):
    """out [nimg P, >= Cc] = relu?(GroupNorm(x)) from stats [nimg, G, 2] (the head of a stats_buffer), every row zero-filled up to its leading dimension.
    split=True: `out` f16 [rows, 3 x block] receives the split A operand rows [hi | hi | lo] (PST_X3H) of the conv that follows"""
    b = _Operands('groupnorm_apply')
    _call('pst_groupnorm_apply', *b.rows('x', x, FMT, nimg * P, Cc), _tc(x), b.ge('stats', stats, F32, nimg * G * 2), b('gamma', gamma, F32, Cc), b('beta', beta, F32, Cc),
          *b.rows('out', out, X3_FMT if split else FMT, nimg * P, 3 * Cc if split else Cc, fill=True), nimg, P, Cc, G, eps, relu, X3H if split else _tc(out))
    return out


class Planes:
    """(hi, lo) 16-bit planes of an fp32 attention operand prepared by the caller (split2): same shape and strides for both"""
    __slots__ = ('hi', 'lo')

    def __init__(self, hi, lo):
        if not (hi.dtype == lo.dtype and hi.shape == lo.shape and hi.stride() == lo.stride()):
            raise RuntimeError('Planes: hi and lo must share dtype, shape and strides, got %s %s %s and %s %s %s' % (hi.dtype, tuple(hi.shape), hi.stride(), lo.dtype, tuple(lo.shape), lo.stride()))
        self.hi, self.lo = hi, lo


def loftup_lr_pe(biases, out, col0, nimg, h, w):
    """the 20 low-res positional features of the h x w token grid into columns [col0, col0 + 20) of every view's rows of `out` [nimg h w, >= col0 + 20]"""
    b = _Operands('loftup_lr_pe')
    _call('pst_loftup_lr_pe', b.ge('biases', biases, F32, 20), *b.rows('out', out, FMT, nimg * h * w, col0 + 20), col0, nimg, h, w, _tc(out))
    return out


# ------------------------------------------------------------------ panoptic post-processing
def pp_scores(logits, cls_threshold, temperature, scores, labels, keep):
    b = _Operands('pp_scores')
    p = b('logits', logits, F32, (-1, -1))
    Q, Ncls = logits.shape
    _call('pst_pp_scores', p, Q, Ncls, float(cls_threshold), float(temperature or 0.0), b.ge('scores', scores, F32, Q), b.ge('labels', labels, I32, Q),
          b.ge('keep', keep, I32, Q))


def pp_scores_softmax(logits, cls_threshold, scores, labels, keep):
    b = _Operands('pp_scores_softmax')
    p = b('logits', logits, F32, (-1, -1))
    Q, Ncls = logits.shape
    _call('pst_pp_scores_softmax', p, Q, Ncls, float(cls_threshold), b.ge('scores', scores, F32, Q), b.ge('labels', labels, I32, Q), b.ge('keep', keep, I32, Q))


def pp_sigmoid(logits, keep, probs, Q, P):
    b = _Operands('pp_sigmoid')
    _call('pst_pp_sigmoid', b.ge('logits', logits, F32, Q * P), b.ge('keep', keep, I32, Q), b.ge('probs', probs, F32, Q * P), Q, P)


def _pp_argmax(what, masks, scores, keep, Q, Hm, Wm, H, W, mask_threshold, best_q, best_m, cnt_orig, cnt_mask):
    b = _Operands(what)
    _call('pst_' + what, b.ge('logits' if what.endswith('logits') else 'probs', masks, F32, Q * Hm * Wm), b.ge('scores', scores, F32, Q), b.ge('keep', keep, I32, Q),
          Q, Hm, Wm, H, W, float(mask_threshold), b.ge('best_q', best_q, I32, H * W), b.ge('best_m', best_m, F32, H * W), b.ge('cnt_orig', cnt_orig, I32, Q),
          b.ge('cnt_mask', cnt_mask, I32, Q))


def pp_argmax(probs, scores, keep, Q, Hm, Wm, H, W, mask_threshold, best_q, best_m, cnt_orig, cnt_mask):
    _pp_argmax('pp_argmax', probs, scores, keep, Q, Hm, Wm, H, W, mask_threshold, best_q, best_m, cnt_orig, cnt_mask)


def pp_fused_fits(Q, Hm, Wm, H, W):
    """host copy of pst_pp_argmax_logits' footprint rule (8x32 output tiles, <= 1024 staged low-res pixels per query)."""
    rh = min(Hm, math.ceil(8 * Hm / H) + 2)
    rw = min(Wm, math.ceil(32 * Wm / W) + 2)
    return 1024 // (rh * rw) >= 1


def pp_argmax_logits(logits, scores, keep, Q, Hm, Wm, H, W, mask_threshold, best_q, best_m, cnt_orig, cnt_mask):
    _pp_argmax('pp_argmax_logits', logits, scores, keep, Q, Hm, Wm, H, W, mask_threshold, best_q, best_m, cnt_orig, cnt_mask)


def pp_select(keep, cnt_orig, cnt_mask, Q, overlap_threshold, keep_out, seg_id):
    b = _Operands('pp_select')
    _call('pst_pp_select', b.ge('keep', keep, I32, Q), b.ge('cnt_orig', cnt_orig, I32, Q), b.ge('cnt_mask', cnt_mask, I32, Q), Q, float(overlap_threshold),
          b.ge('keep_out', keep_out, I32, Q), b.ge('seg_id', seg_id, I32, Q))


def pp_finalize(best_q, best_m, seg_id, n, mask_threshold, void_confidence, pan, conf):
    """seg_id int32 [Q] is read at best_q: the entry point does not take Q, so its length is the caller's"""
    b = _Operands('pp_finalize')
    _call('pst_pp_finalize', b.ge('best_q', best_q, I32, n), b.ge('best_m', best_m, F32, n), b.ge('seg_id', seg_id, I32, 1), n, float(mask_threshold),
          float(void_confidence), b.ge('pan', pan, I32, n), b.ge('conf', conf, F32, n))


# ------------------------------------------------------------------ pointmap post-processing
def pointmap_activate(raw, pts3d, pts3d_local, conf, mode=0):
    b = _Operands('pointmap_activate')
    p = b.ge('raw', raw, F32, 0)
    npix = raw.numel() // 7
    _call('pst_pointmap_activate', p, b.ge('pts3d', pts3d, F32, 3 * npix), b.ge('pts3d_local', pts3d_local, F32, 3 * npix), b.ge('conf', conf, F32, npix), npix, mode)


def focal_weiszfeld(pts3d_local, pp, focal, H, W, iters=10):
    b = _Operands('focal_weiszfeld')
    pf, V = b.sized('focal', focal, F32)
    _call('pst_focal_weiszfeld', b('pts3d_local', pts3d_local, F32, V * H * W * 3), b.ge('pp', pp, F32, 2 * V), pf, V, H, W, iters)
    return focal


def rigid_moments(x, y, conf, out, weight_offset=-1.0):
    b = _Operands('rigid_moments')
    po = b('out', out, F64, (-1, 16))
    V = out.shape[0]
    pc = b.ge('conf', conf, F32, 0)
    npix = conf.numel() // V
    _call('pst_rigid_moments', b.ge('x', x, F32, 3 * V * npix), b.ge('y', y, F32, 3 * V * npix), pc, po, V, npix, float(weight_offset))
    return out


# ------------------------------------------------------------------ QUBO post-processing (engine/postprocess.py:135-336)
def qubo_upsample(logits, probs, Q, hm, wm, H, W):
    b = _Operands('qubo_upsample')
    _call('pst_qubo_upsample', b.ge('logits', logits, F32, Q * hm * wm), b.ge('probs', probs, F32, Q * H * W), Q, hm, wm, H, W)


def qubo_overlap(probs, Q, P, Wacc):
    b = _Operands('qubo_overlap')
    pp = b.ge('probs', probs, F32, Q * P)
    nws = lib().pst_qubo_workspace_floats(Q, P)
    ws = torch.empty(nws, dtype=torch.float32, device=probs.device)
    _call('pst_qubo_overlap', pp, Q, P, b('ws', ws, F32, nws), b.ge('Wacc', Wacc, F64, Q * Q))


def qubo_argmax(probs, sel, P, conf, inst):
    """probs fp32 [Q, P] is read at the rows sel names (ascending, so Q >= their number): the entry point does not take Q"""
    b = _Operands('qubo_argmax')
    ps, nsel = b.sized('sel', sel, I32)
    _call('pst_qubo_argmax', b.ge('probs', probs, F32, nsel * P), ps, nsel, P, b.ge('conf', conf, F32, P), b.ge('inst', inst, I32, P))


# ------------------------------------------------------------------ ASMK retrieval (model/retrieval.py restates the algorithm)
def retrieval_select(x, in_off, out_off, out, max_t, sel_idx=None):
    """per view v (rows [in_off[v], in_off[v+1]) of the fp32 head output x): the out_off[v+1] - out_off[v] rows of largest norm (ties to the lower
    token), in that order, L2-normalised into rows [out_off[v], out_off[v+1]) of out; sel_idx (int32, optional) gets their token indices"""
    b = _Operands('retrieval_select')
    px = b('x', x, F32, (-1, -1), layout='rows')
    pi = b.ge('in_off', in_off, I32, 1)
    V, D = in_off.numel() - 1, x.shape[1]
    _call('pst_retrieval_select', px, x.stride(0), pi, b('out_off', out_off, I32, V + 1), V, int(max_t), D, b('out', out, F32, (-1, D), layout='rows'),
          out.stride(0), b.ge('sel_idx', sel_idx, I32, 0, optional=True))
    return out


def retrieval_nsplit(n, k):
    """centroid-range splits of pst_retrieval_assign: about two workgroups per CU over the row tiles (128 rows), at most one split per 64 centroids"""
    tiles_r, tiles_c = (n + 127) // 128, (k + 63) // 64
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    return max(1, min(tiles_c, (2 * cus + tiles_r - 1) // tiles_r))


def retrieval_assign(x3, c3, cnorm, m, ids, dist, nsplit=None):
    """ids [n, m] / dist [n, m] = the m nearest centroids of each descriptor (ascending ||c||^2 - 2 x.c, ties to the lower index): x3 / c3 the split-f16
    descriptors (split_operand side 0) and centroids (side 1), cnorm fp32 [k].  The partial lists of the centroid splits live in a workspace of this call."""
    b = _Operands('retrieval_assign')
    px = b('x3', x3, X3_FMT, (-1, -1), layout='rows')
    n, K3 = x3.shape
    pc = b('c3', c3, X3_FMT, (-1, K3), layout='rows')
    k = c3.shape[0]
    nsplit = retrieval_nsplit(n, k) if nsplit is None else int(nsplit)
    ws_d = ws_i = None
    if nsplit > 1:
        ws_d = torch.empty(nsplit * n * m, dtype=torch.float32, device=x3.device)
        ws_i = torch.empty(nsplit * n * m, dtype=torch.int32, device=x3.device)
    _call('pst_retrieval_assign', px, x3.stride(0), pc, c3.stride(0), b('cnorm', cnorm, F32, k), n, k, K3, int(m), nsplit,
          b('ws_dist', ws_d, F32, nsplit * n * m, optional=True), b('ws_ids', ws_i, I32, nsplit * n * m, optional=True), b('ids', ids, I32, (n, m)),
          b('dist', dist, F32, (n, m)), _tc(x3))
    return ids, dist


def retrieval_aggregate(x, cent, member, gstart, gword, bits, sums=None):
    """per (view, word) group g: fp32 sum of the residuals x[member] - cent[gword[g]] over members gstart[g] .. gstart[g+1] (ascending) -> packed sign
    bits [G, D / 32] (int32 storage of the uint32 words; bit j of word w = component 32 w + j) and, optionally, the sums [G, D]"""
    b = _Operands('retrieval_aggregate')
    px = b('x', x, F32, (-1, -1), layout='rows')
    (pw, G), D = b.sized('gword', gword, I32), x.shape[1]
    _call('pst_retrieval_aggregate', px, x.stride(0), b('cent', cent, F32, (-1, D), layout='rows'), cent.stride(0), b.ge('member', member, I32, 0),
          b('gstart', gstart, I32, G + 1), pw, G, D, b('sums', sums, F32, (G, D), optional=True), b('bits', bits, I32, (G, D // 32)))
    return bits


def retrieval_scores(q_off, q_word, q_bits, db_off, db_word, db_bits, D, alpha, tau, S, max_q):
    """S [Vq, Vdb] fp32: ASMK binary-kernel similarity of every query view (groups [q_off[i], q_off[i+1]), sorted by word) against every database view"""
    b = _Operands('retrieval_scores')
    pq, pd = b.ge('q_off', q_off, I32, 1), b.ge('db_off', db_off, I32, 1)
    Vq, Vdb = q_off.numel() - 1, db_off.numel() - 1
    _call('pst_retrieval_scores', pq, b.ge('q_word', q_word, I32, 0), b('q_bits', q_bits, I32, (-1, D // 32)), pd, b.ge('db_word', db_word, I32, 0),
          b('db_bits', db_bits, I32, (-1, D // 32)), Vq, Vdb, int(max(1, max_q)), int(D), float(alpha), float(tau), b('S', S, F32, (Vq, Vdb)))
    return S


# ------------------------------------------------------------------ panoptic point cloud (csrc/cloud.hip; engine/cloud.py holds the public entry point)
CLOUD_WG = 1024            # points per workgroup of the count / compact passes
CLOUD_MAX_COLORS = 4096    # colour table rows that fit in LDS
_VIEW_BYTES = C.sizeof(CloudView)


def _view_table(views, cams2world, device, what, absent=()):
    """device table of pst_cloud_view for views = [(conf, pts3d, pts3d_local, img, pan)] (contiguous device tensors, which the caller keeps alive; a
    plane named in `absent` may be None and stays NULL) and cams2world = [V, 3, 4] host floats -> (uint8 tensor, number of workgroups, total number
    of `what`)"""
    tab = (CloudView * len(views))()
    b = _Operands('view table of %s' % what)
    off = wg = 0
    for e, (conf, pts, loc, img, pan), c2w in zip(tab, views, cams2world):
        e.conf = b.ge('conf', conf, F32, 1)
        n = conf.numel()
        e.pts3d, e.pts3d_local = b('pts3d', pts, F32, 3 * n), b('pts3d_local', loc, F32, 3 * n)
        e.img, e.pan = b('img', img, F32, 3 * n, optional='img' in absent), b('pan', pan, I32, n, optional='pan' in absent)
        e.offset, e.npix, e.first_wg = off, n, wg
        e.c2w[:] = [float(x) for row in c2w for x in row]
        off += n
        wg += _wgs(n)
    if off >= 2 ** 31:
        raise RuntimeError('a scene of %d %s exceeds the 2^31 - 1 the kernels of a view table index' % (off, what))
    return torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(device), wg, off


def cloud_view_table(views, cams2world, device):
    """device table of pst_cloud_view for views = [(conf, pts3d, pts3d_local, img, pan)] (contiguous device tensors, which the caller keeps alive)
    and cams2world = [V, 3, 4] host floats -> (uint8 tensor, number of workgroups, total number of points)"""
    return _view_table(views, cams2world, device, 'points')


def cloud_count(table, nviews, nwg, thr, counts):
    b = _Operands('cloud_count')
    _call('pst_cloud_count', b('table', table, U8, nviews * _VIEW_BYTES), nviews, nwg, float(thr), b.ge('counts', counts, I32, nwg))


def cloud_scan(counts, base):
    b = _Operands('cloud_scan')
    _call('pst_cloud_scan', b.ge('counts', counts, I32, 0), counts.numel(), b('base', base, I32, counts.numel() + 1))


def scan_buffers(device, n=None, wg=CLOUD_WG, *, nwg=None):
    """counts [nwg], base [nwg + 1] of one count / cloud_scan / emit compaction over n items in workgroups of wg, or over nwg given -> (nwg, counts, base)"""
    nwg = (n + wg - 1) // wg if nwg is None else nwg
    return nwg, torch.empty(nwg, dtype=torch.int32, device=device), torch.empty(nwg + 1, dtype=torch.int32, device=device)


def cloud_compact(table, nviews, nwg, thr, base, colors, w1, w2, points, points_local, rgb, pan, colors_out, index):
    b = _Operands('cloud_compact')
    pp, n = b.sized('pan', pan, I32)
    _call('pst_cloud_compact', b('table', table, U8, nviews * _VIEW_BYTES), nviews, nwg, float(thr), b('base', base, I32, nwg + 1),
          b('colors', colors, F32, (-1, 3)), colors.shape[0], float(w1), float(w2), b('points', points, F32, 3 * n), b('points_local', points_local, F32, 3 * n),
          b('rgb', rgb, F32, 3 * n), pp, b('colors_out', colors_out, F32, 3 * n), b('index', index, I64, n))


def cloud_segment_median(points_local, pan, m_ptr, id2row, nseg, count, median):
    """count int32 [nseg], median fp32 [nseg, 3] of the rows [0, M) of points_local by segment row (id2row int32, -1 = none); m_ptr = one-element int32
    device tensor holding M"""
    b = _Operands('cloud_segment_median')
    pp, pi = b.ge('pan', pan, I32, 0), b.ge('id2row', id2row, I32, 0)
    _, hist, prefix, rank, nan = _select_workspace(3 * nseg, pan.device, nan=1)
    _call('pst_cloud_segment_median', b('points_local', points_local, F32, 3 * pan.numel()), pp, b.ge('m_ptr', m_ptr, I32, 1), pan.numel(), pi, id2row.numel(),
          nseg, b('hist', hist, I32, 1536 * nseg), b('prefix', prefix, I32, 6 * nseg), b('rank', rank, I32, 6 * nseg), b('nan', nan, I32, 3 * nseg),
          b('count', count, I32, nseg), b('median', median, F32, 3 * nseg))


# ------------------------------------------------------------------ QUBO mask selection (csrc/qubo_solve.hip; engine/postprocess.py holds the public entry points)
def qubo_anneal_max_n():
    """the largest problem the device annealer takes (W in the LDS of one CU)"""
    return lib().pst_qubo_anneal_max_n()


def qubo_anneal(W, replicas, num_iters, T0, T_end, lambda_reg, seed, x_all, e_all, best_x, best_e):
    """`replicas` independent simulated anneals of E(x) = x^T W x + lambda_reg mean(x) (W fp32 [N, N]) -> x_all uint8 [replicas, N], e_all fp32 [replicas],
    best_x uint8 [N], best_e fp32 [1]; a pure function of its arguments (include/panst3r_hip.h).  An N the kernel does not take raises, outputs untouched."""
    b = _Operands('qubo_anneal')
    pw = b('W', W, F32, (-1, -1))
    N = W.shape[0]
    b.require(W.shape[1] == N, 'W must be square, got %s', tuple(W.shape))
    _call('pst_qubo_anneal', pw, N, int(replicas), int(num_iters), float(T0), float(T_end), float(lambda_reg), int(seed) & (2 ** 64 - 1),
          b('x_all', x_all, U8, replicas * N), b('e_all', e_all, F32, replicas), b('best_x', best_x, U8, N), b('best_e', best_e, F32, 1))


# ------------------------------------------------------------------ voxel fusion of the point cloud (csrc/voxel.hip; engine/voxels.py holds the public entry point)
VOXEL_MERGE = 1            # merge runs of equal keys inside a wave before the global atomics (A/B: tools/voxel_bench.py, docs/experiments.md)


def voxel_capacity(M):
    """slots of the two open-addressing tables: the next power of two >= 2 M"""
    return 1 << max(1, (2 * int(M) - 1).bit_length())


def voxel_workspace(M, device):
    """the initialised workspaces of one fusion of M points (include/panst3r_hip.h): dict of device tensors"""
    cap = voxel_capacity(M)
    i32 = dict(dtype=torch.int32, device=device)
    i64 = dict(dtype=torch.int64, device=device)
    return {'cap': cap, 'keys': torch.full((cap,), -1, **i64), 'first': torch.full((cap,), 2 ** 31 - 1, **i32), 'slot_rank': torch.empty(cap, **i32),
            'point_slot': torch.empty(M, **i32), 'first_row': torch.empty(M, **i32), 'cnt': torch.zeros(M, **i32), 'sums': torch.zeros(M, 6, **i64),
            'pair_keys': torch.full((cap,), -1, **i64), 'pair_cnt': torch.zeros(cap, **i32), 'best': torch.zeros(M, **i64), 'status': torch.zeros(2, **i32)}


def voxel_insert(points, inv, ws, merge=None):
    b = _Operands('voxel_insert')
    pts = b.rows3('points', points, F32)
    _call('pst_voxel_insert', *pts, float(inv), b('keys', ws['keys'], I64, ws['cap']), ws['cap'], b.ge('first', ws['first'], I32, ws['cap']),
          b('point_slot', ws['point_slot'], I32, pts[1]), b.ge('status', ws['status'], I32, 2), int(VOXEL_MERGE if merge is None else merge))


def voxel_count(ws, counts):
    """the capacity of `first` is no argument of the entry point: a table of M points has at least 2 M slots"""
    b = _Operands('voxel_count')
    ps, M = b.sized('point_slot', ws['point_slot'], I32)
    _call('pst_voxel_count', ps, b.ge('first', ws['first'], I32, 2 * M), M, b('counts', counts, I32, _wgs(M)))


def voxel_rank(ws, base):
    b = _Operands('voxel_rank')
    ps, M = b.sized('point_slot', ws['point_slot'], I32)
    _call('pst_voxel_rank', ps, b.ge('first', ws['first'], I32, 2 * M), M, b('base', base, I32, _wgs(M) + 1), b.ge('slot_rank', ws['slot_rank'], I32, 2 * M),
          b.ge('first_row', ws['first_row'], I32, M))


def voxel_accumulate(points, rgb, pan, inv, id2row, ws, point_voxel, merge=None):
    b = _Operands('voxel_accumulate')
    (pp, M), cap = b.sized('pan', pan, I32), ws['cap']
    _call('pst_voxel_accumulate', b('points', points, F32, 3 * M), b('rgb', rgb, F32, 3 * M), pp, M, float(inv), b('point_slot', ws['point_slot'], I32, M),
          b.ge('slot_rank', ws['slot_rank'], I32, cap), b.ge('id2row', id2row, I32, 0), id2row.numel(), b.ge('cnt', ws['cnt'], I32, M),
          b.ge('sums', ws['sums'], I64, 6 * M), b.ge('pair_keys', ws['pair_keys'], I64, cap), b.ge('pair_cnt', ws['pair_cnt'], I32, cap), cap,
          b('point_voxel', point_voxel, I32, M), b.ge('status', ws['status'], I32, 2), int(VOXEL_MERGE if merge is None else merge))


def voxel_vote(ws):
    """best int64 [M] is written at the rows the pair keys name: the entry point does not take M"""
    b = _Operands('voxel_vote')
    _call('pst_voxel_vote', b.ge('pair_keys', ws['pair_keys'], I64, ws['cap']), b.ge('pair_cnt', ws['pair_cnt'], I32, ws['cap']), ws['cap'],
          b.ge('best', ws['best'], I64, 1))


def voxel_emit(points, index, mv_ptr, inv, voxel_size, ws, colors, w1, w2, out_points, out_rgb, out_pan, out_colors, out_votes, out_first):
    b = _Operands('voxel_emit')
    pi, M = b.sized('index', index, I64)
    _call('pst_voxel_emit', b.ge('points', points, F32, 3 * M), pi, b('first_row', ws['first_row'], I32, M), b.ge('mv_ptr', mv_ptr, I32, 1), M, float(inv),
          float(voxel_size), b.ge('cnt', ws['cnt'], I32, M), b.ge('sums', ws['sums'], I64, 6 * M), b.ge('best', ws['best'], I64, M),
          b('colors', colors, F32, (-1, 3)), colors.shape[0], float(w1), float(w2), b('out_points', out_points, F32, 3 * M), b('out_rgb', out_rgb, F32, 3 * M),
          b('out_pan', out_pan, I32, M), b('out_colors', out_colors, F32, 3 * M), b('out_votes', out_votes, I32, M), b('out_first', out_first, I64, M))


# ------------------------------------------------------------------ connected components of the voxels (csrc/components.hip; engine/voxels.py holds the public entry points)
VCC_MERGE = 1              # reduce runs of adjacent lanes with one root inside a wave before vcc_flatten's atomics (A/B: tests/diag/vcc_bench.py, docs/experiments.md)
VCC_FULL, VCC_DUPLICATE, VCC_RANGE, VCC_LOOP = 1, 2, 4, 8      # PST_VCC_*: the bits of status[0]


def vcc_cells(points, first_row, mv_ptr, inv, cells):
    """cells int32 [M, 3]: rows [0, *mv_ptr) = the integer cell of every voxel's first point (first_row: the fusion's workspace)"""
    b = _Operands('vcc_cells')
    pf, M = b.sized('first_row', first_row, I32)
    _call('pst_vcc_cells', b('points', points, F32, 3 * M), pf, b.ge('mv_ptr', mv_ptr, I32, 1), M, float(inv), b('cells', cells, I32, 3 * M))


def vcc_pair_capacity(Mv, nids):
    """slots of the vote table: twice the min(nids, 26) Mv distinct (component, id) pairs that can occur, a power of two (2^31 at the most)"""
    return min(voxel_capacity(max(1, min(int(nids), 26)) * int(Mv)), 1 << 31)


def vcc_workspace(Mv, device, pairs=0):
    """the initialised workspaces of one labelling of Mv voxels (include/panst3r_hip.h): dict of device tensors; pairs > 0 adds the vote table"""
    cap = voxel_capacity(Mv)
    i32 = dict(dtype=torch.int32, device=device)
    i64 = dict(dtype=torch.int64, device=device)
    ws = {'cap': cap, 'keys': torch.full((cap,), -1, **i64), 'rows': torch.empty(cap, **i32), 'parent': torch.empty(Mv, **i32), 'root': torch.empty(Mv, **i32),
          'size': torch.zeros(Mv, **i32), 'points': torch.zeros(Mv, **i64), 'lo': torch.full((Mv, 3), 2 ** 31 - 1, **i32), 'hi': torch.full((Mv, 3), -2 ** 31, **i32),
          'rank_of': torch.empty(Mv, **i32), 'status': torch.zeros(4, **i32)}
    if pairs:
        ws.update(pair_cap=pairs, pair_keys=torch.full((pairs,), -1, **i64), pair_cnt=torch.zeros(pairs, **i32), best=torch.zeros(Mv, **i64))
    return ws


def _vcc_voxels(b, cells, pan):
    """-> (cells, pan, Mv): the three leading arguments of the entry points over cells int32 [Mv, 3] and pan int32 [Mv]"""
    pp, Mv = b.sized('pan', pan, I32)
    return b('cells', cells, I32, (Mv, 3)), pp, Mv


def vcc_build(cells, pan, ws):
    b = _Operands('vcc_build')
    vox = _vcc_voxels(b, cells, pan)
    _call('pst_vcc_build', *vox, b('keys', ws['keys'], I64, ws['cap']), b('rows', ws['rows'], I32, ws['cap']), ws['cap'], b('parent', ws['parent'], I32, vox[2]),
          b.ge('status', ws['status'], I32, 4))


def vcc_link(cells, pan, connectivity, ws):
    b = _Operands('vcc_link')
    vox = _vcc_voxels(b, cells, pan)
    _call('pst_vcc_link', *vox, b.ge('keys', ws['keys'], I64, ws['cap']), b.ge('rows', ws['rows'], I32, ws['cap']), ws['cap'], int(connectivity),
          b('parent', ws['parent'], I32, vox[2]), b.ge('status', ws['status'], I32, 4))


def vcc_flatten(count, cells, ws, merge=None):
    b = _Operands('vcc_flatten')
    pc, Mv = b.sized('count', count, I32)
    _call('pst_vcc_flatten', b('parent', ws['parent'], I32, Mv), pc, b('cells', cells, I32, 3 * Mv), Mv, b('root', ws['root'], I32, Mv),
          b('size', ws['size'], I32, Mv), b('points', ws['points'], I64, Mv), b('lo', ws['lo'], I32, 3 * Mv), b('hi', ws['hi'], I32, 3 * Mv),
          b.ge('status', ws['status'], I32, 4), int(VCC_MERGE if merge is None else merge))


def vcc_count(ws, counts):
    b = _Operands('vcc_count')
    Mv = ws['root'].numel()
    _call('pst_vcc_count', b('root', ws['root'], I32, Mv), Mv, b('counts', counts, I32, _wgs(Mv)))


def vcc_rank(pan, ws, base, component, table):
    """component int32 [Mv]; table: dict of root, pan, size int32 [Mv], points int64 [Mv], cell_lo, cell_hi int32 [Mv, 3] - rows [0, C) are written"""
    b = _Operands('vcc_rank')
    pp, Mv = b.sized('pan', pan, I32)
    _call('pst_vcc_rank', b('root', ws['root'], I32, Mv), pp, Mv, b('base', base, I32, _wgs(Mv) + 1), b.ge('size', ws['size'], I32, Mv),
          b.ge('points', ws['points'], I64, Mv), b.ge('lo', ws['lo'], I32, 3 * Mv), b.ge('hi', ws['hi'], I32, 3 * Mv), b.ge('rank_of', ws['rank_of'], I32, Mv),
          b('component', component, I32, Mv), b('table root', table['root'], I32, Mv), b('table pan', table['pan'], I32, Mv),
          b('table size', table['size'], I32, Mv), b('table points', table['points'], I64, Mv), b('table cell_lo', table['cell_lo'], I32, 3 * Mv),
          b('table cell_hi', table['cell_hi'], I32, 3 * Mv))


def vcc_votes(cells, pan, connectivity, min_voxels, ws):
    b = _Operands('vcc_votes')
    vox = _vcc_voxels(b, cells, pan)
    _call('pst_vcc_votes', vox[0], vox[1], b('root', ws['root'], I32, vox[2]), b.ge('size', ws['size'], I32, vox[2]), vox[2], b.ge('keys', ws['keys'], I64, ws['cap']),
          b.ge('rows', ws['rows'], I32, ws['cap']), ws['cap'], int(connectivity), int(min_voxels), b('pair_keys', ws['pair_keys'], I64, ws['pair_cap']),
          b('pair_cnt', ws['pair_cnt'], I32, ws['pair_cap']), ws['pair_cap'], b.ge('status', ws['status'], I32, 4))


def vcc_apply(pan, min_voxels, rgb, colors, w1, w2, ws, out_pan, out_colors):
    b = _Operands('vcc_apply')
    pp, Mv = b.sized('pan', pan, I32)
    _call('pst_vcc_apply', pp, b('root', ws['root'], I32, Mv), b.ge('size', ws['size'], I32, Mv), b('best', ws['best'], I64, Mv), Mv, int(min_voxels),
          b('rgb', rgb, F32, 3 * Mv), b('colors', colors, F32, (-1, 3)), colors.shape[0], float(w1), float(w2), b('out_pan', out_pan, I32, Mv),
          b('out_colors', out_colors, F32, 3 * Mv), b.ge('status', ws['status'], I32, 4))


# ------------------------------------------------------------------ z-buffered rendering of a cloud (csrc/render.hip; engine/render.py holds the public entry points)
RENDER_PRECHECK = 1        # read the z-buffer cell before the atomic and skip one that cannot win (A/B: tests/diag/render_bench.py, docs/experiments.md)
RENDER_CAM_FLOATS = 16     # floats per camera of the device table: twelve world-to-camera numbers, f, cx, cy, near
RENDER_MAX_RADIUS = 16     # PST_RENDER_MAX_RADIUS (pst_render_max_radius() of the built library; tests/test_render_host.py holds the three together)


def render_max_radius():
    """PST_RENDER_MAX_RADIUS: the largest footprint radius the splat kernel takes"""
    return lib().pst_render_max_radius()


def render_splat(points, cams, H, W, half_size, radius, max_radius, zbuf, precheck=None):
    """atomicMin of every point's key into zbuf int64 [B, H, W] (cleared to all ones by the caller) for the B cameras of cams fp32 [B, 16]"""
    b = _Operands('render_splat')
    pts, pc = b.rows3('points', points, F32), b('cams', cams, F32, (-1, RENDER_CAM_FLOATS))
    B = cams.shape[0]
    _call('pst_render_splat', *pts, pc, B, int(H), int(W), float(half_size), int(radius), int(max_radius), b('zbuf', zbuf, I64, (B, H, W)),
          int(RENDER_PRECHECK if precheck is None else precheck))


def render_resolve(zbuf, rgb, colors, pan, index, depth, out_pan, out_rgb, out_colors):
    """per cell of zbuf: the winner's row, depth, pan, rgb and colours (an empty cell: -1 and zeros)"""
    b = _Operands('render_resolve')
    (pz, n), (pp, M) = b.sized('zbuf', zbuf, I64), b.sized('pan', pan, I32)
    _call('pst_render_resolve', pz, n, M, b('rgb', rgb, F32, 3 * M), b('colors', colors, F32, 3 * M), pp, b('index', index, I64, n), b('depth', depth, F32, n),
          b('out_pan', out_pan, I32, n), b('out_rgb', out_rgb, F32, 3 * n), b('out_colors', out_colors, F32, 3 * n))


# ------------------------------------------------------------------ cross-view depth consistency (csrc/consistency.hip; engine/consistency.py holds the public entry points)
def consist_view_table(views, cams2world, cams, shapes, device):
    """the three device tables of the consistency kernels for views = [(conf, pts3d, pts3d_local, pan or None)] (contiguous device tensors, which the
    caller keeps alive), cams2world = [V, 3, 4] host floats, cams = float32 [V, 16] host (engine.render.camera_table of every view's own camera) and
    shapes = [(H, W)] -> (pst_cloud_view table as a uint8 tensor - img is not read and stays NULL -, cams tensor, dims int32 [V, 2], number of
    workgroups, total number of pixels)"""
    b = _Operands('consist_view_table')
    b.require(len(views) == len(cams2world) == len(shapes) == len(cams) > 0 and tuple(cams.shape) == (len(views), RENDER_CAM_FLOATS),
              'one camera-to-world matrix, one row of cams float32 [V, %d] and one shape per view, V >= 1' % RENDER_CAM_FLOATS)
    table, wg, off = _view_table([(conf, pts, loc, None, pan) for conf, pts, loc, pan in views], cams2world, device, 'pixels', absent=('img', 'pan'))
    b.require(all(v[0].numel() == int(H) * int(W) for v, (H, W) in zip(views, shapes)), 'every view holds the H W pixels of its shape')
    dims = torch.tensor([(int(H), int(W)) for H, W in shapes], dtype=torch.int32).reshape(-1, 2)
    return table, torch.from_numpy(cams).contiguous().to(device), dims.to(device), wg, off


def _consist_tables(b, table, cams, nviews):
    """-> (table, cams): the scene's view table and its cameras float32 [nviews, 16], the two leading arguments of the consistency entry points"""
    return b('table', table, U8, nviews * _VIEW_BYTES), b('cams', cams, F32, (nviews, RENDER_CAM_FLOATS))


def consist_depth(table, cams, nviews, nwg, thr, local, depth):
    """depth fp32 [N]: every pixel's depth in its own camera, 0 where the view measured nothing (conf < thr, a non-finite point, nearer than near)"""
    b = _Operands('consist_depth')
    pd, N = b.sized('depth', depth, F32)
    _call('pst_consist_depth', *_consist_tables(b, table, cams, nviews), nviews, nwg, N, float(thr), int(bool(local)), pd)


def consist_count(table, cams, dims, nviews, nwg, rel_tol, local, depth, agree, violate, same_label=None):
    """agree, violate, same_label (or None: no panoptic id is read) int32 [N] of every pixel against every other view's depth"""
    b = _Operands('consist_count')
    pd, N = b.sized('depth', depth, F32)
    _call('pst_consist_count', *_consist_tables(b, table, cams, nviews), b('dims', dims, I32, (nviews, 2)), nviews, nwg, N, float(rel_tol), int(bool(local)), pd,
          b('agree', agree, I32, N), b('violate', violate, I32, N), b('same_label', same_label, I32, N, optional=True))


# ------------------------------------------------------------------ one fused TSDF surface out of all views (csrc/tsdf.hip; engine/tsdf.py holds the public entry points)
TSDF_FULL, TSDF_RANGE = 1, 4       # PST_TSDF_*: the bits of status[0]
TSDF_MAX_BAND = 4                  # PST_TSDF_MAX_BAND
TSDF_MAX_PAIRS = 2 ** 30 - 1       # what the count / rank kernels take


def tsdf_pairs(Mv, band):
    """the (voxel row, offset) pairs of Mv voxels at `band`: Mv (2 band)^3"""
    return int(Mv) * (2 * int(band)) ** 3


def tsdf_capacity(Mv, band):
    """slots of the node table: the next power of two >= twice the pairs"""
    return voxel_capacity(tsdf_pairs(Mv, band))


def tsdf_table_bytes(Mv, band):
    """device memory of the node table of one fusion: keys (8), first and slot_rank (4 + 4) per slot, pair_slot and first_pair (4 + 4) per pair"""
    return 16 * tsdf_capacity(Mv, band) + 8 * tsdf_pairs(Mv, band)


def tsdf_workspace(Mv, band, device):
    """the initialised workspaces of the node table of Mv voxels at `band` (include/panst3r_hip.h): dict of device tensors.  The names are those of
    `voxel_workspace`, so that `voxel_count` / `voxel_rank` rank the nodes: a pair is a point there, a node a voxel."""
    P = tsdf_pairs(Mv, band)
    cap = tsdf_capacity(Mv, band)
    i32 = dict(dtype=torch.int32, device=device)
    return {'cap': cap, 'keys': torch.full((cap,), -1, dtype=torch.int64, device=device), 'first': torch.full((cap,), 2 ** 31 - 1, **i32),
            'slot_rank': torch.empty(cap, **i32), 'point_slot': torch.empty(P, **i32), 'first_row': torch.empty(P, **i32), 'status': torch.zeros(4, **i32)}


def tsdf_insert(cells, band, ws):
    b = _Operands('tsdf_insert')
    vox = b.rows3('cells', cells, I32)
    _call('pst_tsdf_insert', *vox, int(band), b('keys', ws['keys'], I64, ws['cap']), ws['cap'], b('first', ws['first'], I32, ws['cap']),
          b('point_slot', ws['point_slot'], I32, tsdf_pairs(vox[1], band)), b.ge('status', ws['status'], I32, 4))


def tsdf_nodes(cells, band, Nn, ws, nodes, voxel_row):
    """nodes int32 [Nn, 3] in rank order; voxel_row int32 [Nn] (filled with -1 by the caller): the voxel whose cell is the node"""
    b = _Operands('tsdf_nodes')
    vox = b.rows3('cells', cells, I32)
    _call('pst_tsdf_nodes', *vox, int(band), b('first_row', ws['first_row'], I32, tsdf_pairs(vox[1], band)), Nn, b.ge('keys', ws['keys'], I64, ws['cap']), ws['cap'],
          b.ge('slot_rank', ws['slot_rank'], I32, ws['cap']), b('nodes', nodes, I32, (Nn, 3)), b('voxel_row', voxel_row, I32, Nn), b.ge('status', ws['status'], I32, 4))


def tsdf_integrate(nodes, voxel_size, band, table, cams, dims, nviews, depth, sdf, weight):
    """sdf fp32 [Nn], weight int32 [Nn] of the nodes against the depth planes of `consist_depth` (table, cams, dims: `consist_view_table`); depth fp32
    [N] holds the scene's pixels, which the view table counts on the device"""
    b = _Operands('tsdf_integrate')
    nd = b.rows3('nodes', nodes, I32)
    _call('pst_tsdf_integrate', *nd, float(voxel_size), int(band), *_consist_tables(b, table, cams, nviews), b('dims', dims, I32, (nviews, 2)), nviews,
          b.ge('depth', depth, F32, 1), b('sdf', sdf, F32, nd[1]), b('weight', weight, I32, nd[1]))


def _tsdf_nodes(b, nodes, ws):
    """-> (nodes, Nn, keys, cap, slot_rank): the five leading arguments of the entry points over the ranked nodes int32 [Nn, 3] and their table"""
    return (*b.rows3('nodes', nodes, I32), b('keys', ws['keys'], I64, ws['cap']), ws['cap'], b('slot_rank', ws['slot_rank'], I32, ws['cap']))


def tsdf_cells(nodes, ws, sdf, weight, min_weight, cell_vertex, counts):
    """cell_vertex int32 [Nn]: 1 where the cell at the node is a surface cell, else 0; counts [ceil(Nn / 1024)]"""
    b = _Operands('tsdf_cells')
    tab = _tsdf_nodes(b, nodes, ws)
    Nn = tab[1]
    _call('pst_tsdf_cells', *tab, b('sdf', sdf, F32, Nn), b('weight', weight, I32, Nn), int(min_weight), b('cell_vertex', cell_vertex, I32, Nn),
          b('counts', counts, I32, _wgs(Nn)), b.ge('status', ws['status'], I32, 4))


def tsdf_vertices(nodes, ws, sdf, weight, min_weight, voxel_row, vox_count, vox_pan, vox_colors, voxel_size, base, cell_vertex, vertices, vertex_ids, colors):
    """vertices fp32 [Nv, 3], vertex_ids int32 [Nv], colors fp32 [Nv, 3] in rank order; cell_vertex becomes the vertex row of every node's cell, or -1"""
    b = _Operands('tsdf_vertices')
    tab = _tsdf_nodes(b, nodes, ws)
    Nn, (pp, Mv), (pi, Nv) = tab[1], b.sized('vox_pan', vox_pan, I32), b.sized('vertex_ids', vertex_ids, I32)
    _call('pst_tsdf_vertices', *tab, b('sdf', sdf, F32, Nn), b('weight', weight, I32, Nn), int(min_weight), b('voxel_row', voxel_row, I32, Nn),
          b('vox_count', vox_count, I32, Mv), pp, b('vox_colors', vox_colors, F32, 3 * Mv), Mv, float(voxel_size), b('base', base, I32, _wgs(Nn) + 1),
          b('cell_vertex', cell_vertex, I32, Nn), b('vertices', vertices, F32, 3 * Nv), pi, b('colors', colors, F32, 3 * Nv), b.ge('status', ws['status'], I32, 4))


def tsdf_face_count(nodes, ws, sdf, weight, min_weight, cell_vertex, face_mask, counts):
    """face_mask int32 [Nn]: bit a = the lattice edge from the node along axis a emits two triangles; counts [ceil(Nn / 1024)] in faces"""
    b = _Operands('tsdf_face_count')
    tab = _tsdf_nodes(b, nodes, ws)
    Nn = tab[1]
    _call('pst_tsdf_face_count', *tab, b('sdf', sdf, F32, Nn), b('weight', weight, I32, Nn), int(min_weight), b('cell_vertex', cell_vertex, I32, Nn),
          b('face_mask', face_mask, I32, Nn), b('counts', counts, I32, _wgs(Nn)), b.ge('status', ws['status'], I32, 4))


def tsdf_face_emit(nodes, ws, sdf, cell_vertex, face_mask, vertex_ids, base, faces, face_ids, edge):
    """faces int32 [>= F, 3], face_ids int32, edge int64 [>= F]: rows [0, F) are written, F = base[-1] <= 6 Nv"""
    b = _Operands('tsdf_face_emit')
    tab = _tsdf_nodes(b, nodes, ws)
    Nn, (pv, Nv) = tab[1], b.sized('vertex_ids', vertex_ids, I32)
    pf, cap = b.sized('face_ids', face_ids, I32, 6 * Nv)
    _call('pst_tsdf_face_emit', *tab, b('sdf', sdf, F32, Nn), b('cell_vertex', cell_vertex, I32, Nn), b('face_mask', face_mask, I32, Nn), pv,
          b('base', base, I32, _wgs(Nn) + 1), b('faces', faces, I32, 3 * cap), pf, b('edge', edge, I64, cap), b.ge('status', ws['status'], I32, 4))


# ------------------------------------------------------------------ z-buffered rasterisation of a labelled mesh (csrc/mesh.hip; engine/mesh.py holds the public entry points)
MESH_PRECHECK = 0          # RENDER_PRECHECK's relaxed load before the atomic: OFF here - a mesh has a few samples per pixel, most atomics win, and the load
                           # only adds to them (0.87 against 0.56 ms for 16 cameras: tests/diag/mesh_bench.py, docs/experiments.md §6l)
MESH_CAM_FLOATS = RENDER_CAM_FLOATS    # floats per camera of the device table: twelve world-to-camera numbers, fx, fy, cx, cy
MESH_LANE_PIXELS = 64      # PST_MESH_LANE_PIXELS (pst_mesh_lane_pixels() of the built library; tests/test_mesh_host.py holds the three together)
MESH_BIG_CAPACITY = 1 << 22    # the most (camera, face) entries the list of large faces gets (8 bytes each); beyond it a large face stays with its lane


def mesh_lane_pixels():
    """PST_MESH_LANE_PIXELS: the largest pixel bounding box one lane rasterises; a larger face goes to the one-wave-per-face path"""
    return lib().pst_mesh_lane_pixels()


def mesh_workspace(B, Nf, device, capacity=None):
    """the list of large faces of one pst_mesh_raster launch over B cameras and Nf faces: {'big': int64 [capacity], 'count': int64 [1]}.  `count` is
    cleared before every launch (mesh_raster does it)."""
    cap = min(int(B) * int(Nf), MESH_BIG_CAPACITY) if capacity is None else int(capacity)
    return {'big': torch.empty(max(cap, 1), dtype=torch.int64, device=device), 'count': torch.zeros(1, dtype=torch.int64, device=device), 'capacity': cap}


def _mesh(b, vertices, faces):
    """-> (vertices, Nv, faces, F): the four consecutive arguments of the entry points over a mesh of vertices fp32 [Nv, 3] and faces int32 [F, 3]"""
    return (*b.rows3('vertices', vertices, F32), *b.rows3('faces', faces, I32))


def mesh_raster(vertices, faces, cams, H, W, near, far, zbuf, ws, precheck=None):
    """atomicMin of every covered sample's key into zbuf int64 [B, H, W] (cleared to all ones by the caller) for the B cameras of cams fp32 [B, 16];
    ws = mesh_workspace(...)"""
    b = _Operands('mesh_raster')
    mesh, pc = _mesh(b, vertices, faces), b('cams', cams, F32, (-1, MESH_CAM_FLOATS))
    B = cams.shape[0]
    b.require(ws['capacity'] >= 0, 'the capacity of the list of large faces is not negative')
    out = (b('zbuf', zbuf, I64, (B, H, W)), b.ge('big', ws['big'], I64, ws['capacity']), b('count', ws['count'], I64, 1))
    ws['count'].zero_()
    _call('pst_mesh_raster', *mesh, pc, B, int(H), int(W), float(near), float(far), *out, ws['capacity'], int(MESH_PRECHECK if precheck is None else precheck))


def mesh_resolve(zbuf, vertices, faces, cams, near, vertex_ids, face_ids, face, depth, pan):
    """per cell of zbuf int64 [B, H, W]: the winning face, its depth and its id (face_ids, the nearest corner's vertex_ids, or 0); an empty cell: -1, 0, 0"""
    b = _Operands('mesh_resolve')
    pz, mesh = b('zbuf', zbuf, I64, (-1, -1, -1)), _mesh(b, vertices, faces)
    (B, H, W), n = zbuf.shape, zbuf.numel()
    _call('pst_mesh_resolve', pz, B, H, W, *mesh, b('cams', cams, F32, (B, MESH_CAM_FLOATS)), float(near), b('vertex_ids', vertex_ids, I32, mesh[1], optional=True),
          b('face_ids', face_ids, I32, mesh[3], optional=True), b('face', face, I64, n), b('depth', depth, F32, n), b('pan', pan, I32, n))


def _mesh_area_args(b, pan, id2row, counts):
    """-> (pan, B, H W, id2row, ntab, S, counts): the seven leading arguments of the two area entry points"""
    pp, pc = b('pan', pan, I32, (-1, -1, -1)), b('counts', counts, I32, (pan.shape[0], -1))
    b.require(counts.shape[1] >= 1, 'counts int32 [B, S] needs S >= 1')
    return pp, pan.shape[0], pan.shape[1] * pan.shape[2], b.ge('id2row', id2row, I32, 0), id2row.numel(), counts.shape[1], pc


def mesh_area_count(pan, id2row, counts):
    """counts int32 [B, S] (cleared by the caller) += the pixels of pan int32 [B, H, W] per (camera, listed id)"""
    _call('pst_mesh_area_count', *_mesh_area_args(_Operands('mesh_area_count'), pan, id2row, counts))


def mesh_area_apply(pan, id2row, counts, min_area, out):
    """out = pan where the id is listed and has at least min_area pixels in its camera, else 0"""
    b = _Operands('mesh_area_apply')
    args = _mesh_area_args(b, pan, id2row, counts)
    po = b('out', out, I32, tuple(pan.shape))
    b.require(po != args[0], 'out is not pan')
    _call('pst_mesh_area_apply', *args, int(min_area), po)


# ------------------------------------------------------------------ mesh shading: vertex normals, interpolated attributes, a headlight shade (csrc/mesh_normals.hip and the
# end of csrc/mesh.hip; engine/shade.py holds the public entry points)
MESH_INTERP_MAX_CHANNELS = 16      # PST_MESH_INTERP_MAX_CHANNELS
MESH_NORMALS_MAX_SHIFT = 1100      # PST_MESH_NORMALS_MAX_SHIFT
MESH_SHADE_NONE, MESH_SHADE_FLAT, MESH_SHADE_SMOOTH = 0, 1, 2      # PST_MESH_SHADE_*


def mesh_normals(vertices, faces, sh, acc, out):
    """out fp32 [Nv, 3] = the area-weighted unit normals of vertices fp32 [Nv, 3] over faces int32 [Nf, 3], (0, 0, 0) for a vertex on no valid face;
    sh: the scale exponent of the contract's step 3 (engine/shade.py computes it); acc int64 [Nv, 3, 2]: the two-limb sums, cleared here"""
    b = _Operands('mesh_normals')
    mesh = _mesh(b, vertices, faces)
    Nv = mesh[1]
    b.require(isinstance(sh, int) and not isinstance(sh, bool) and abs(sh) <= MESH_NORMALS_MAX_SHIFT, 'sh is an int with |sh| <= %d, got %r', MESH_NORMALS_MAX_SHIFT, sh)
    pa, po = b('acc', acc, I64, (Nv, 3, 2)), b('out', out, F32, (Nv, 3))
    acc.zero_()
    _call('pst_mesh_normals_accumulate', *mesh, sh, pa)
    _call('pst_mesh_normals_finish', pa, Nv, po)


def mesh_interp(face, vertices, faces, cams, near, *, attr=None, fill=0.0, out_attr=None, shade_mode=MESH_SHADE_NONE, normals=None, out_shade=None):
    """per pixel of face int64 [B, H, W] (MeshRender.face, or any values): out_attr fp32 [B, H, W, C] = attr fp32 [Nv, C] interpolated perspective-correctly
    over the pixel's face, `fill` on a miss; out_shade fp32 [B, H, W] = the headlight shade of the face's normal (shade_mode MESH_SHADE_FLAT) or of the
    interpolated normals fp32 [Nv, 3] (MESH_SHADE_SMOOTH), 0 on a miss.  Either output or both."""
    b = _Operands('mesh_interp')
    pf = b('face', face, I64, (-1, -1, -1))                                   # raises unless face is a 3-D tensor: the shape is read after it
    B, H, W = face.shape
    mesh = _mesh(b, vertices, faces)
    Nv, pc = mesh[1], b('cams', cams, F32, (B, MESH_CAM_FLOATS))
    b.require(shade_mode in (MESH_SHADE_NONE, MESH_SHADE_FLAT, MESH_SHADE_SMOOTH), 'shade_mode is 0 (none), 1 (flat) or 2 (smooth), got %r', shade_mode)
    b.require((attr is None) == (out_attr is None), 'attr and out_attr go together')
    b.require((shade_mode != MESH_SHADE_NONE) == (out_shade is not None), 'out_shade goes with a shade mode (mode %d)', shade_mode)
    b.require((shade_mode == MESH_SHADE_SMOOTH) == (normals is not None), 'normals go with the smooth shade mode, and it needs them (mode %d)', shade_mode)
    b.require(attr is not None or out_shade is not None, 'neither attributes nor a shade asked for')
    nc = 0
    if attr is not None:
        nc = int(attr.shape[1]) if isinstance(attr, torch.Tensor) and attr.dim() == 2 else 0
        b.require(1 <= nc <= MESH_INTERP_MAX_CHANNELS, 'attr is fp32 [Nv, C] with 1 <= C <= %d, got %s', MESH_INTERP_MAX_CHANNELS,
                  tuple(attr.shape) if isinstance(attr, torch.Tensor) else type(attr).__name__)
        b.require(isinstance(fill, (int, float)) and not isinstance(fill, bool) and math.isfinite(fill) and abs(fill) <= 3.4028234663852886e38, 'fill must be a finite float32, got %r', fill)
    pa, po = b('attr', attr, F32, (Nv, nc), optional=True), b('out_attr', out_attr, F32, (B, H, W, nc), optional=True)
    pn, ps = b('normals', normals, F32, (Nv, 3), optional=True), b('out_shade', out_shade, F32, (B, H, W), optional=True)
    _call('pst_mesh_interp', pf, B, H, W, *mesh, pc, float(near), pa, nc, float(fill), po, int(shade_mode), pn, ps)


# ------------------------------------------------------------------ panoptic evaluation (csrc/evaluate.hip; engine/evaluate.py holds the public entry point)
EVAL_MERGE = 1                      # add runs of equal (slab, row, column) keys inside a wave with one atomic (A/B: tests/diag/eval_bench.py, docs/experiments.md)
EVAL_MAX_TABLE_BYTES = 256 << 20    # the largest `counts` table [slabs, P+1, G+1] int32 that panoptic_quality allocates
EVAL_MAX_ID = 1 << 24               # segment ids are below this (a COCO panoptic id is 24 bits of an RGB triple): bounds the id -> row tables


def pq_count(pred, gt, slab_off, id2row_p, id2row_g, P, G, counts, merge=None):
    """counts int32 [S, P+1, G+1] (cleared by the caller) += the pixels of pred / gt int32 [N] per (slab, row, column); slab_off int64 [S + 1]"""
    b = _Operands('pq_count')
    (pp, N), (ps, S1) = b.sized('pred', pred, I32), b.sized('slab_off', slab_off, I64, 2)
    _call('pst_pq_count', pp, b('gt', gt, I32, N), N, ps, S1 - 1,b.ge('id2row_p', id2row_p, I32, 0), id2row_p.numel(), b.ge('id2row_g', id2row_g, I32, 0),
          id2row_g.numel(), int(P), int(G), b('counts', counts, I32, (S1 - 1, P + 1, G + 1)), int(EVAL_MERGE if merge is None else merge))


def pq_match(counts, cat_p, cat_g, pred_area, gt_area, match, iou, pred_state):
    """areas, match / iou per (slab, gt column) and the state per (slab, predicted row) of a counts table [S, P+1, G+1]; an operand of P (or G) rows
    is NULL when P (or G) is 0"""
    b = _Operands('pq_match')
    pc = b('counts', counts, I32, (-1, -1, -1))
    S, P, G = counts.shape[0], counts.shape[1] - 1, counts.shape[2] - 1
    nz = lambda p, rows: p if rows else None
    _call('pst_pq_match', pc, S, P, G, nz(b('cat_p', cat_p, I32, P), P), nz(b('cat_g', cat_g, I32, G), G), nz(b('pred_area', pred_area, I32, (S, P)), S * P),
          nz(b('gt_area', gt_area, I32, (S, G)), S * G), nz(b('match', match, I32, (S, G)), S * G), nz(b('iou', iou, F64, (S, G)), S * G),
          nz(b('pred_state', pred_state, I32, (S, P)), S * P))


# ------------------------------------------------------------------ surface mesh of the pointmap grids (csrc/surface.hip; engine/surface.py holds the public entry points)
SURFACE_WG = 256                    # PST_SURFACE_WG: quads (count / emit) or faces (islands) per workgroup, one per thread
SURFACE_MAX_PIXELS = 1 << 30        # scenes beyond this are refused: the face count (two per quad) stays inside int32


def surface_dims(shapes, device):
    """device table int32 [V, 4] = (H, W, first_wg, 0) of the quad kernels for views of the shapes (H, W) -> (tensor, number of workgroups)"""
    rows, wg = [], 0
    for H, W in shapes:
        rows.append((int(H), int(W), wg, 0))
        wg += _wgs(max(H - 1, 0) * max(W - 1, 0), SURFACE_WG)
    return torch.tensor(rows, dtype=torch.int32).reshape(-1, 4).to(device), wg


def surface_rows(index, N, row):
    """row int32 [N]: the cloud row of every scene pixel (index int64 [M] of the cloud), -1 for a pixel that was filtered out"""
    b = _Operands('surface_rows')
    pi = b.ge('index', index, I64, 0)
    b.require(index.numel() <= N, 'index holds %d rows of a scene of %d pixels', index.numel(), N)
    _call('pst_surface_rows', pi if index.numel() else None, index.numel(), N, b('row', row, I32, N))


def _surface_quads(b, table, dims, nviews, nwg, row):
    """-> (table, dims, nviews, nwg, row): the five leading arguments of the quad entry points; row int32 [N] over the pixels the view table counts"""
    b.require(nwg > 0, 'a scene without quads')
    return b('table', table, U8, nviews * _VIEW_BYTES), b('dims', dims, I32, (nviews, 4)), nviews, nwg, b.ge('row', row, I32, 1)


def surface_count(table, dims, nviews, nwg, row, k, counts):
    """counts int32 [nwg]: the faces of every workgroup's quads (table: the cloud's view table, dims: `surface_dims`, k = float32(1 + max_depth_ratio) or inf)"""
    b = _Operands('surface_count')
    _call('pst_surface_count', *_surface_quads(b, table, dims, nviews, nwg, row), float(k), b('counts', counts, I32, nwg))


def surface_emit(table, dims, nviews, nwg, row, k, vertex_ids, base, faces, face_ids, quad):
    """faces int32 [., 3], face_ids int32 [.], quad int64 [.]: rows [0, base[nwg]) are written; each holds two rows per quad of the scene; vertex_ids
    int32 holds the cloud's rows, which `row` names"""
    b = _Operands('surface_emit')
    quads, (pf, cap) = _surface_quads(b, table, dims, nviews, nwg, row), b.sized('face_ids', face_ids, I32, 2 * SURFACE_WG * nwg)
    _call('pst_surface_emit', *quads, float(k), b.ge('vertex_ids', vertex_ids, I32, 1), b('base', base, I32, nwg + 1), b('faces', faces, I32, 3 * cap), pf,
          b('quad', quad, I64, cap))


def surface_workspace(M, device):
    """parent, size int32 [M] (initialised by surface_link) and the zeroed status word of one labelling of a mesh on M vertex rows"""
    return {'parent': torch.empty(M, dtype=torch.int32, device=device), 'size': torch.empty(M, dtype=torch.int32, device=device),
            'status': torch.zeros(1, dtype=torch.int32, device=device)}


def _surface_faces(b, faces, ws):
    """-> (faces, F, M): the three leading arguments of the island entry points over faces int32 [F, 3] on M vertex rows"""
    pf, F = b.rows3('faces', faces, I32)
    b.require(F > 0 and ws['parent'].numel() > 0, 'a mesh without faces or vertex rows')
    return pf, F, ws['parent'].numel()


def surface_link(faces, ws):
    b = _Operands('surface_link')
    mesh = _surface_faces(b, faces, ws)
    _call('pst_surface_link', *mesh, b('parent', ws['parent'], I32, mesh[2]), b('size', ws['size'], I32, mesh[2]), b.ge('status', ws['status'], I32, 1))


def surface_components(faces, ws, component):
    """component int32 [F] = the smallest vertex row of every face's component; ws['size'][root] = the component's faces"""
    b = _Operands('surface_components')
    mesh = _surface_faces(b, faces, ws)
    _call('pst_surface_components', *mesh, b('parent', ws['parent'], I32, mesh[2]), b('component', component, I32, mesh[1]), b('size', ws['size'], I32, mesh[2]),
          b.ge('status', ws['status'], I32, 1))


def surface_keep_count(component, ws, min_faces, counts):
    """ws['size'] int32 [M] is read at the roots `component` names: the entry point does not take M"""
    b = _Operands('surface_keep_count')
    pc, F = b.sized('component', component, I32)
    _call('pst_surface_keep_count', pc, b.ge('size', ws['size'], I32, 1), F, int(min_faces), b('counts', counts, I32, _wgs(F, SURFACE_WG)))


def surface_keep_emit(faces, face_ids, quad, component, ws, min_faces, base, out_faces, out_face_ids, out_quad):
    """the faces whose component has at least min_faces faces, in their order -> rows [0, base[-1]) of the outputs (each as long as its input)"""
    b = _Operands('surface_keep_emit')
    pf, F, M = _surface_faces(b, faces, ws)
    _call('pst_surface_keep_emit', pf, b('face_ids', face_ids, I32, F), b('quad', quad, I64, F), b('component', component, I32, F), b('size', ws['size'], I32, M), F,
          int(min_faces), b('base', base, I32, _wgs(F, SURFACE_WG) + 1), b('out_faces', out_faces, I32, 3 * F), b('out_face_ids', out_face_ids, I32, F),
          b('out_quad', out_quad, I64, F))


# ------------------------------------------------------------------ mesh simplification by vertex clustering (csrc/simplify.hip; engine/simplify.py holds the public entry points)
SIMPLIFY_MERGE = 1                  # let the first lane of a run of adjacent faces with one key probe for the run (same results)
SIMPLIFY_FULL, SIMPLIFY_RANGE = 1, 4                 # PST_SIMPLIFY_*: the bits of status[0]
SIMPLIFY_MAX_KEYED = 2 ** 21 - 2    # the new vertices a 3 x 21-bit face key takes (dedupe)
SIMPLIFY_STATUS_WORDS = 8


def simplify_workspace(M, F, device):
    """used int32 [M] (zeroed), face_slot int32 [F] and the zeroed status words of one simplification; `simplify_table` adds the face table"""
    return {'used': torch.zeros(M, dtype=torch.int32, device=device), 'face_slot': torch.empty(F, dtype=torch.int32, device=device),
            'status': torch.zeros(SIMPLIFY_STATUS_WORDS, dtype=torch.int32, device=device), 'cap': 0, 'keys': None, 'winner': None}


def simplify_table(ws):
    """the initialised open-addressing table of the faces (dedupe): keys all ones, winner INT32_MAX, capacity the next power of two >= 2 F"""
    F, dev = ws['face_slot'].numel(), ws['face_slot'].device
    ws['cap'] = voxel_capacity(F)
    ws['keys'] = torch.full((ws['cap'],), -1, dtype=torch.int64, device=dev)
    ws['winner'] = torch.full((ws['cap'],), 2 ** 31 - 1, dtype=torch.int32, device=dev)
    return ws


def _simplify_status(b, ws):
    return b('status', ws['status'], I32, SIMPLIFY_STATUS_WORDS)


def simplify_used(faces, ws):
    """ws['used'][v] = 1 for every vertex row a face names; a corner outside the rows sets SIMPLIFY_RANGE"""
    b = _Operands('simplify_used')
    pf, F = b.rows3('faces', faces, I32)
    pu, M = b.sized('used', ws['used'], I32)
    b.require(F > 0 and M > 0, 'a mesh without faces or vertex rows')
    _call('pst_simplify_used', pf, F, M, pu, _simplify_status(b, ws))


def simplify_mask(vertices, ws, masked):
    """masked fp32 [M, 3] = the used vertices, NaN for the others; status[1] += the used vertices"""
    b = _Operands('simplify_mask')
    pv, M = b.rows3('vertices', vertices, F32)
    b.require(M > 0, 'a mesh without vertex rows')
    _call('pst_simplify_mask', pv, b('used', ws['used'], I32, M), M, b('masked', masked, F32, 3 * M), _simplify_status(b, ws))


def simplify_remap(faces, cluster, Mv, dedupe, ws, merge=None):
    """ws['face_slot'] int32 [F]: every face's slot in the face table (0 without dedupe), -1 left out, -2 degenerate; status[2 .. 4] count the faces
    left out, degenerate and remaining"""
    b = _Operands('simplify_remap')
    pf, F = b.rows3('faces', faces, I32)
    pc, M = b.sized('cluster', cluster, I32)
    b.require(F > 0 and 0 < Mv <= M, 'a mesh without faces, or %d new vertices of %d', Mv, M)
    cap = ws['cap'] if dedupe else 0
    b.require(not dedupe or cap >= 2 * F, 'dedupe without a face table (simplify_table) of at least 2 F slots')
    _call('pst_simplify_remap', pf, F, M, pc, int(Mv), int(bool(dedupe)), b('keys', ws['keys'], I64, cap) if dedupe else None, cap,
          b('winner', ws['winner'], I32, cap) if dedupe else None, b('face_slot', ws['face_slot'], I32, F), _simplify_status(b, ws),
          int(SIMPLIFY_MERGE if merge is None else merge))


def simplify_count(dedupe, ws, counts):
    b = _Operands('simplify_count')
    ps, F = b.sized('face_slot', ws['face_slot'], I32, 1)
    _call('pst_simplify_count', ps, b('winner', ws['winner'], I32, ws['cap']) if dedupe else None, F, int(bool(dedupe)),
          b('counts', counts, I32, _wgs(F, SURFACE_WG)))


def simplify_emit(faces, quad, cluster, vertex_ids, Mv, dedupe, ws, base, out_faces, out_face_ids, out_quad, src_face):
    """the surviving faces in their order -> rows [0, base[-1]) of the outputs (each F rows); vertex_ids int32: the NEW vertices' ids, at least Mv"""
    b = _Operands('simplify_emit')
    pf, F = b.rows3('faces', faces, I32)
    pc, M = b.sized('cluster', cluster, I32)
    b.require(F > 0 and 0 < Mv <= M, 'a mesh without faces, or %d new vertices of %d', Mv, M)
    _call('pst_simplify_emit', pf, b('quad', quad, I64, F), pc, b.ge('vertex_ids', vertex_ids, I32, Mv), b('face_slot', ws['face_slot'], I32, F),
          b('winner', ws['winner'], I32, ws['cap']) if dedupe else None, F, M, int(Mv), int(bool(dedupe)), b('base', base, I32, _wgs(F, SURFACE_WG) + 1),
          b('out_faces', out_faces, I32, 3 * F), b('out_face_ids', out_face_ids, I32, F), b('out_quad', out_quad, I64, F), b('src_face', src_face, I32, F))


# ------------------------------------------------------------------ 3-D scores: mesh surface sampler and fixed-radius nearest neighbour (csrc/nearest.hip; engine/score3d.py holds the public entry points)
MESH_SAMPLE_MAX_SUBDIV = 1 << 15    # PST_MESH_SAMPLE_MAX_SUBDIV
MESH_SAMPLE_MAX_TOTAL = 2 ** 31 - 256
MESH_SAMPLE_TOTAL = 1               # PST_MESH_SAMPLE_TOTAL: the bit of the sampler's status[0]
NN_FULL, NN_LISTS = 1, 2            # PST_NN_*: the bits of the search's status[0]
NN_MAX_POINTS = 1 << 30


def mesh_sample_count(vertices, faces, spacing, max_subdiv, counts, total, status):
    """counts int32 [F]; total int64 [1] and status int32 [4] zeroed by the caller (include/panst3r_hip.h)"""
    b = _Operands('mesh_sample_count')
    mesh = _mesh(b, vertices, faces)
    _call('pst_mesh_sample_count', *mesh, float(spacing), int(max_subdiv), b('counts', counts, I32, mesh[3]), b('total', total, I64, 1), b('status', status, I32, 4))


def mesh_sample_emit(vertices, faces, prefix, total, vertex_ids, face_ids, points, face, ids, status):
    """the outputs' rows are the capacity: a `total` beyond them is refused before the launch"""
    b = _Operands('mesh_sample_emit')
    (pv, Nv, pf, F), (pface, capacity) = _mesh(b, vertices, faces), b.sized('face', face, I32)
    _call('pst_mesh_sample_emit', pv, Nv, pf, F, b('prefix', prefix, I32, F + 1), int(total), capacity, b('vertex_ids', vertex_ids, I32, Nv, optional=True),
          b('face_ids', face_ids, I32, F, optional=True), b('points', points, F32, 3 * capacity), pface, b('ids', ids, I32, capacity), b('status', status, I32, 4))


def _lists_workspace(n, device, slot_name):
    """the initialised cell table and per-cell lists of n entries (csrc/voxel_table.h): dict of device tensors; `start` is made by the caller"""
    cap = voxel_capacity(n)
    i32 = dict(dtype=torch.int32, device=device)
    return {'cap': cap, 'keys': torch.full((cap,), -1, dtype=torch.int64, device=device), 'cell_count': torch.zeros(cap, **i32), 'start': None,
            'fill': torch.zeros(cap, **i32), slot_name: torch.empty(n, **i32), 'rows': torch.empty(n, **i32)}


def _lists(b, ws, n):
    """-> (keys, cap, start, cell_count, rows): the five consecutive arguments of the entry points that search the built lists `ws` of n entries"""
    return (b.ge('keys', ws['keys'], I64, ws['cap']), ws['cap'], b.ge('start', ws['start'], I32, ws['cap']),
            b.ge('cell_count', ws['cell_count'], I32, ws['cap']), b('rows', ws['rows'], I32, n))


def nn_workspace(M, device):
    """the initialised workspaces of one search structure over M targets (include/panst3r_hip.h): dict of device tensors"""
    return dict(_lists_workspace(M, device, 'point_slot'), status=torch.zeros(4, dtype=torch.int32, device=device))


def nn_insert(targets, inv, ws):
    b = _Operands('nn_insert')
    tg = b.rows3('targets', targets, F32)
    _call('pst_nn_insert', *tg, float(inv), b('keys', ws['keys'], I64, ws['cap']), ws['cap'], b('cell_count', ws['cell_count'], I32, ws['cap']),
          b('point_slot', ws['point_slot'], I32, tg[1]), b.ge('status', ws['status'], I32, 4))


def nn_scatter(ws):
    """ws['start'] = the exclusive prefix sum of ws['cell_count'] (int32 [cap]), made by the caller"""
    b = _Operands('nn_scatter')
    M, cap = ws['point_slot'].numel(), ws['cap']
    _call('pst_nn_scatter', b('point_slot', ws['point_slot'], I32, M), M, b('start', ws['start'], I32, cap), b.ge('cell_count', ws['cell_count'], I32, cap),
          b('fill', ws['fill'], I32, cap), b('rows', ws['rows'], I32, M), b.ge('status', ws['status'], I32, 4))


def nn_query(queries, targets, inv, r2, ws, max_cell_points, d2, row):
    b = _Operands('nn_query')
    q, tg = b.rows3('queries', queries, F32), b.rows3('targets', targets, F32)
    keys, cap, start, cell_count, rows = _lists(b, ws, tg[1])
    _call('pst_nn_query', *q, *tg, float(inv), float(r2), keys, cap, start, cell_count, rows, int(max_cell_points), b('d2', d2, F32, q[1]), b('row', row, I32, q[1]),
          b.ge('status', ws['status'], I32, 4))


# ------------------------------------------------------------------ one fused ICP step (csrc/nearest.hip; engine/score3d.py's icp / refine_alignment)
ICP_CHUNK, ICP_LANES, ICP_MOMENTS = 4096, 256, 20      # PST_ICP_CHUNK, PST_ICP_LANES, PST_ICP_MOMENTS: the fixed order of the sums (tests/icp_ref.py reads them here)


def icp_workspace(N, device, moments=ICP_MOMENTS):
    """the workspaces of `icp_step` over N source points: partials double [ceil(N / ICP_CHUNK), 20], out double [20], status int32 [4] (zeroed here;
    the caller clears it between steps if it reads it per step)"""
    return {'N': int(N), 'partials': torch.empty(_wgs(int(N), ICP_CHUNK), moments, dtype=torch.float64, device=device),
            'out': torch.empty(moments, dtype=torch.float64, device=device), 'status': torch.zeros(4, dtype=torch.int32, device=device)}


def _icp_sums(b, iws, N, moments):
    """-> (partials, out, status): the three trailing arguments of the two ICP steps over N source points, `moments` doubles per row"""
    b.require(iws['N'] == N, 'the workspace is one of %d source points, the call has %d', iws['N'], N)
    return (b('partials', iws['partials'], F64, _wgs(N, ICP_CHUNK) * moments), b('out', iws['out'], F64, moments), b('status', iws['status'], I32, 4))


def icp_step(source, A, targets, inv, cell_r2, r2, ws, max_cell_points, iws, d2=None, row=None):
    """one fused ICP step (include/panst3r_hip.h): `source` moved by the 3 x 4 matrix A (12 numbers, rounded to fp32 here), searched in the built
    structure `ws` of `targets` (cell edge 1 / inv, cell_r2 = its squared edge), accepted within r2 <= cell_r2 -> iws['out'] double [20]; d2 / row
    [N] are written when given (both or neither).  A larger r2 raises ValueError: the 27 cells would not hold every match."""
    b = _Operands('icp_step')
    src, tg = b.rows3('source', source, F32), b.rows3('targets', targets, F32)
    A = [float(a) for a in (A.reshape(-1).tolist() if hasattr(A, 'reshape') else A)]
    if len(A) != 12:
        raise ValueError('icp_step takes a 3 x 4 matrix, got %d numbers' % len(A))
    if not float(r2) <= float(cell_r2):
        raise ValueError('icp_step: the squared radius %g exceeds the squared cell edge %g of the search structure' % (r2, cell_r2))
    if (d2 is None) != (row is None):
        raise ValueError('icp_step: d2 and row go together')
    b.require(lib().pst_icp_chunk() == ICP_CHUNK, 'the library does not sum in the chunks of %d the workspaces are made for', ICP_CHUNK)
    keys, cap, start, cell_count, rows = _lists(b, ws, tg[1])
    _call('pst_icp_step', *src, *A, *tg, float(inv), float(r2), keys, cap, start, cell_count, rows, int(max_cell_points),
          b('d2', d2, F32, src[1], optional=True), b('row', row, I32, src[1], optional=True), *_icp_sums(b, iws, src[1], ICP_MOMENTS))
    return iws['out']


# ------------------------------------------------------------------ the exact distance to a triangle mesh within a radius (csrc/meshdist.hip; engine/meshdist.py holds the public entry points)
MESHDIST_FULL, MESHDIST_LISTS, MESHDIST_TOTAL = 1, 2, 4      # PST_MESHDIST_*: the bits of status[0]
MESHDIST_FACE_CAP = 2 ** 31 - 1                              # PST_MESHDIST_FACE_CAP
MESHDIST_MAX = 1 << 30                                       # queries, faces and pairs of one call


def meshdist_count(vertices, faces, inv, counts, total, status):
    """counts int32 [F]; total int64 [1] and status int32 [4] zeroed by the caller (include/panst3r_hip.h)"""
    b = _Operands('meshdist_count')
    mesh = _mesh(b, vertices, faces)
    _call('pst_meshdist_count', *mesh, float(inv), b('counts', counts, I32, mesh[3]), b('total', total, I64, 1), b('status', status, I32, 4))


def meshdist_workspace(P, device):
    """the initialised workspaces of one index of P (face, cell) pairs (include/panst3r_hip.h): dict of device tensors"""
    return dict(_lists_workspace(P, device, 'pair_slot'), P=int(P))


def meshdist_insert(vertices, faces, inv, prefix, ws, status):
    """the workspaces' rows are `total`: a prefix that ends elsewhere sets MESHDIST_TOTAL and nothing is written"""
    b = _Operands('meshdist_insert')
    mesh = _mesh(b, vertices, faces)
    _call('pst_meshdist_insert', *mesh, float(inv), b('prefix', prefix, I32, mesh[3] + 1), ws['P'], b('keys', ws['keys'], I64, ws['cap']), ws['cap'],
          b('cell_count', ws['cell_count'], I32, ws['cap']), b('pair_slot', ws['pair_slot'], I32, ws['P']), b('status', status, I32, 4))


def meshdist_scatter(prefix, ws, status):
    """ws['start'] = the exclusive prefix sum of ws['cell_count'] (int32 [cap]), made by the caller"""
    b = _Operands('meshdist_scatter')
    pp, P, cap = b.ge('prefix', prefix, I32, 1), ws['P'], ws['cap']
    _call('pst_meshdist_scatter', b.ge('pair_slot', ws['pair_slot'], I32, P), pp, prefix.numel() - 1, P, b('start', ws['start'], I32, cap),
          b.ge('cell_count', ws['cell_count'], I32, cap), b('fill', ws['fill'], I32, cap), b('rows', ws['rows'], I32, P), b('status', status, I32, 4))


def meshdist_query(queries, vertices, faces, inv, r2, ws, max_cell_faces, d2, face, closest, status):
    """d2 fp32 [Nq], face int32 [Nq], closest fp32 [Nq, 3] or None"""
    b = _Operands('meshdist_query')
    q, mesh = b.rows3('queries', queries, F32), _mesh(b, vertices, faces)
    _call('pst_meshdist_query', *q, *mesh, float(inv), float(r2), *_lists(b, ws, ws['P']), ws['P'], int(max_cell_faces), b('d2', d2, F32, q[1]),
          b('face', face, I32, q[1]), b('closest', closest, F32, 3 * q[1], optional=True), b('status', status, I32, 4))


# ------------------------------------------------------------------ one fused point-to-plane ICP step against the triangles (csrc/meshdist.hip; engine/meshdist.py's icp_to_mesh)
ICP_PLANE_MOMENTS = 40      # PST_ICP_PLANE_MOMENTS: doubles per row of partials and in out (the order of the sums is ICP_CHUNK / ICP_LANES, as icp_step's)


def icp_plane_workspace(N, device):
    """the workspaces of `icp_plane_step` over N source points: `icp_workspace` with 40 doubles per row of partials and in out"""
    return icp_workspace(N, device, ICP_PLANE_MOMENTS)


def icp_plane_step(source, A, c0, vertices, faces, inv, cell_r2, r2, ws, max_cell_faces, iws, d2=None, face=None):
    """one fused point-to-plane step (include/panst3r_hip.h): `source` moved by the 3 x 4 matrix A (12 numbers, rounded to fp32 here), searched in the
    built lists `ws` of the mesh (cell edge 1 / inv, cell_r2 = its squared edge), accepted within r2 <= cell_r2, the normal equations about the centre
    c0 (3 numbers) -> iws['out'] double [40]; d2 / face [N] are written when given (both or neither).  A larger r2 raises ValueError: the lists
    would not hold every match."""
    b = _Operands('icp_plane_step')
    src, mesh = b.rows3('source', source, F32), _mesh(b, vertices, faces)
    A = [float(a) for a in (A.reshape(-1).tolist() if hasattr(A, 'reshape') else A)]
    c0 = [float(c) for c in (c0.reshape(-1).tolist() if hasattr(c0, 'reshape') else c0)]
    if len(A) != 12 or len(c0) != 3:
        raise ValueError('icp_plane_step takes a 3 x 4 matrix and a centre of 3 numbers, got %d and %d numbers' % (len(A), len(c0)))
    if not float(r2) <= float(cell_r2):
        raise ValueError('icp_plane_step: the squared radius %g exceeds the squared cell edge %g of the search structure' % (r2, cell_r2))
    if (d2 is None) != (face is None):
        raise ValueError('icp_plane_step: d2 and face go together')
    _call('pst_plane_icp_step', *src, *A, *c0, *mesh, float(inv), float(r2), *_lists(b, ws, ws['P']), ws['P'], int(max_cell_faces),
          b('d2', d2, F32, src[1], optional=True), b('face', face, I32, src[1], optional=True), *_icp_sums(b, iws, src[1], ICP_PLANE_MOMENTS))
    return iws['out']


# ------------------------------------------------------------------ depth evaluation against ground truth (csrc/depth_eval.hip; engine/depth_eval.py holds the public entry point)
DEPTH_VIEW_WORDS, DEPTH_MOMENTS = 8, 16      # PST_DEPTH_VIEW_WORDS, PST_DEPTH_MOMENTS
DEPTH_MAX_THRESHOLDS = 4


class DepthTable:
    """the view table of the depth-evaluation entry points: `host` int64 [V, 8] (numpy; the refusals read it), `dev` the same rows on the device (the
    kernels read it), `slab_rows` int32 [S + 1] on the device, and the tensors the rows point into, kept alive here"""

    def __init__(self, rows, slabs, device, keep=()):
        import numpy as np
        self.host = np.zeros((len(rows), DEPTH_VIEW_WORDS), dtype=np.int64)
        blocks, edges = 0, [0]
        for v, ((pred, stride, gt, conf, npix), slab) in enumerate(zip(rows, slabs)):
            if v and slab != slabs[v - 1]:
                edges.append(blocks)
            self.host[v] = (pred, stride, gt, conf or 0, npix, blocks, slab, 0)
            blocks += (npix + ICP_CHUNK - 1) // ICP_CHUNK
        edges.append(blocks)
        self.nviews, self.nblocks, self.nslabs, self.keep = len(rows), blocks, len(edges) - 1, keep
        blob = torch.from_numpy(np.concatenate([self.host.reshape(-1), np.array(edges, dtype=np.int64)])).to(device)      # one copy
        self.dev, self.slab_rows = blob[:self.host.size], blob[self.host.size:].to(torch.int32)

    def _args(self, b):
        """the four leading arguments of the entry points"""
        return b('views', self.dev, I64, self.nviews * DEPTH_VIEW_WORDS), self.host.ctypes.data, self.nviews, self.nblocks


def depth_table(views, slabs, device):
    """views = [(pred, stride, gt, conf or None)]: fp32 device tensors, pred read at the element stride `stride` from its first element, gt and conf
    contiguous; slabs = the slab of every view, ascending from 0 by steps of 0 or 1 -> DepthTable"""
    rows, keep = [], []
    b = _Operands('depth_table')
    for pred, stride, gt, conf in views:
        pp, (pg, npix) = b('pred', pred, F32, 1, True, layout='any'), b.sized('gt', gt, F32)
        reach = pred.untyped_storage().nbytes() // pred.element_size() - pred.storage_offset()
        b.require(int(stride) >= 1 and reach >= (npix - 1) * int(stride) + 1, 'pred is read at %d elements with the stride %s from its first element: '
                  'its storage holds %d from there', npix, stride, reach)
        rows.append((pp, int(stride), pg, b('conf', conf, F32, npix, optional=True), npix))
        keep += [pred, gt, conf]
    return DepthTable(rows, [int(s) for s in slabs], device, keep)


def depth_median_workspace(table, device):
    """the zeroed int32 workspace of depth_median: hist [S, 2, 2, 256], prefix [S, 2, 2] and rank [S, 2, 2] in one allocation; a call leaves it zeroed"""
    return _select_workspace(2 * table.nslabs, device)[0]


def depth_median(table, min_depth, max_depth, conf_thr, count, median, ws=None):
    """count int32 [S], median fp32 [S, 2] = the exact medians (of pred, of gt) over the valid pixels of every slab; ws = a `depth_median_workspace`
    that is all zero (a call leaves it so), or None for a fresh one"""
    b = _Operands('depth_median')
    S, pc = table.nslabs, b('count', count, I32, table.nslabs)
    b('ws', ws, I32, S * 1032, optional=True)
    _, hist, prefix, rank, _ = _select_workspace(2 * S, count.device, ws=ws)
    _call('pst_depth_median', *table._args(b), S, float(min_depth), float(max_depth), float(conf_thr), b('hist', hist, I32, 1024 * S), b('prefix', prefix, I32, 4 * S),
          b('rank', rank, I32, 4 * S), pc, b('median', median, F32, 2 * S))


def depth_workspace(table, device):
    """partials double [nblocks, 16] and out double [S, 16] of depth_moments / depth_errors"""
    return {'partials': torch.empty(table.nblocks, DEPTH_MOMENTS, dtype=torch.float64, device=device),
            'out': torch.empty(table.nslabs, DEPTH_MOMENTS, dtype=torch.float64, device=device)}


def depth_moments(table, min_depth, max_depth, conf_thr, ws):
    """ws['out'][s, :5] = n, sum p, sum g, sum pp, sum pg over the valid pixels of slab s, in the fixed order of the contract"""
    b = _Operands('depth_moments')
    _call('pst_depth_moments', *table._args(b), b('slab_rows', table.slab_rows, I32, table.nslabs + 1), table.nslabs, float(min_depth), float(max_depth),
          float(conf_thr), b('partials', ws['partials'], F64, table.nblocks * DEPTH_MOMENTS), b('out', ws['out'], F64, table.nslabs * DEPTH_MOMENTS))


def depth_errors(table, min_depth, max_depth, conf_thr, align, thresholds, ws):
    """ws['out'][s, :5 + K] = n, sum |d|/g, sum dd/g, sum dd, sum |d| and the inlier counts of the K thresholds under p' = align[s, 0] p + align[s, 1]"""
    b = _Operands('depth_errors')
    t = [float(x) for x in thresholds]
    _call('pst_depth_errors', *table._args(b), b('slab_rows', table.slab_rows, I32, table.nslabs + 1), table.nslabs, float(min_depth), float(max_depth),
          float(conf_thr), b('align', align, F64, 2 * table.nslabs), len(t), *(t + [0.0] * DEPTH_MAX_THRESHOLDS)[:DEPTH_MAX_THRESHOLDS],
          b('partials', ws['partials'], F64, table.nblocks * DEPTH_MOMENTS), b('out', ws['out'], F64, table.nslabs * DEPTH_MOMENTS))      # (K > 4: the library refuses)
