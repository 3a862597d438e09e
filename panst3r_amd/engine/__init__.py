"""Mirror of the reference's `panst3r.engine` exports that are on (or next to) the hot path:
`from panst3r_amd.engine import panoptic_inference_v2` replaces `from panst3r.engine import panoptic_inference_v2`
(engine/__init__.py, tools/demo_panst3r.py:41)."""
from .postprocess import panoptic_inference_v2, panoptic_inference_v1, panoptic_inference_qubo, solve_qubo_device  # noqa: F401
from . import pointmaps  # noqa: F401,E402  (pointmap post-processing: postprocess / estimate_focal_knowing_depth / rigid_points_registration)
from .images import load_images  # noqa: F401,E402
from .retrieval import PanSt3RRetriever  # noqa: F401,E402  (keyframe selection by retrieval, reference engine/retrieval.py)
from .cloud import panoptic_point_cloud, PanopticCloud, default_colors, camera_frusta  # noqa: F401,E402  (the scene's labelled point cloud, demo :279-300, :622-687)
from .voxels import voxelize_cloud, VoxelCloud, VoxelComponents, voxel_components, clean_voxel_labels  # noqa: F401,E402  (voxel fusion of the cloud with multi-view label votes; not in the reference)
from .render import render_cloud, render_cameras, orbit_cameras, CloudRender  # noqa: F401,E402  (the cloud seen from any camera: depth, panoptic map, colours; not in the reference)
from .consistency import view_consistency, ViewConsistency  # noqa: F401,E402  (f14: every pixel checked against every other view's depth - agreeing views, views that see through it, agreeing labels - and the floater filter PanopticCloud.filter_consistent; not in the reference)
from .evaluate import panoptic_quality  # noqa: F401,E402  (PQ / SQ / RQ and mIoU of panoptic maps against ground truth, per scene or per view; not in the reference)
from .mesh import render_mesh, ground_truth_maps, mesh_camera_table, load_ply_mesh, panoptic_vertex_ids, MeshRender  # noqa: F401,E402  (ground-truth depth and panoptic maps rasterised from a labelled mesh; reference tools/preprocess_scannetpp.py:395-494 through OpenGL)
from .shade import vertex_normals, interpolate_render, shade_render  # noqa: F401,E402  (f17: area-weighted vertex normals, per-vertex attributes interpolated over a MeshRender, a headlight shade - colour and shaded views of every mesh, PanopticMesh.render_color; not in the reference)
from .surface import panoptic_mesh, PanopticMesh  # noqa: F401,E402  (the pointmap grids triangulated into one labelled surface mesh on the cloud's rows; not in the reference)
from .score3d import sample_mesh, nearest_points, similarity_from_cameras, score_reconstruction, MeshSamples  # noqa: F401,E402  (a reconstruction scored against a ground-truth mesh in 3-D: F-score, chamfer, a panoptic quality on the surface; not in the reference)
from .score3d import icp, refine_alignment, Alignment  # noqa: F401,E402  (the alignment to the ground truth refined on the geometry by ICP, one fused kernel per step; not in the reference)
from .meshdist import mesh_distance, icp_to_mesh  # noqa: F401,E402  (icp_to_mesh: point-to-plane ICP against the triangles, f13; mesh_distance: the exact distance from points to a triangle mesh within a radius - squared distance, face, closest point - behind score_reconstruction(metric='surface'); not in the reference)
from .depth_eval import depth_quality  # noqa: F401,E402  (f16: predicted depths against ground-truth depths on the device - AbsRel, SqRel, RMSE, MAE, delta < t after a median / least-squares alignment, per view or per scene; not in the reference)
from .camera_eval import camera_quality  # noqa: F401,E402  (f16: predicted cameras against ground-truth cameras - RRA, RTA, mAA, ATE, focal error; host float64; not in the reference)
from .tsdf import fuse_surface, FusedMesh  # noqa: F401,E402  (f15:the views fused in a truncated signed distance volume and ONE surface extracted by surface nets - PanopticCloud.fused_mesh; not in the reference)
from .simplify import simplify_mesh, SimplifiedMesh  # noqa: F401,E402  (f18: any mesh made smaller by vertex clustering on the voxel grid - one vertex per cell with the voted id, collapsed and coinciding faces removed - PanopticMesh.simplify; not in the reference)
