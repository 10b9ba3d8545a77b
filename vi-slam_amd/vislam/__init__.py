"""vislam -- thin ctypes binding over the C ABI of libvislam_hip.so (include/vislam_hip.h).

This is plumbing for tests and bench.py; the product is the shared library.  The classes here
mirror the reference's surface for the hot path (names, argument meaning, error behaviour):

  Context.orb_detect_compute   <-> CameraGPU::detectAndComputeGPUFeatures  (src/CameraGPU.cpp:71-117)
  Context.bf_knn2_hamming      <-> MatcherGPU::computeGPUMatches           (src/MatcherGPU.cpp:44-66)
  Context.good_matches         <-> Matcher::computeBestMatches             (src/Matcher.cpp:353-367)
  Context.essential_ransac / recover_pose <-> VISystem::EstimatePoseFeaturesRansac (src/VISystem.cpp:1679-1701)
  Context.f2f_ransac           <-> VISystem::F2FRansac                      (src/VISystem.cpp:612-769)
  Context.f2f_batch / batch_f2f                       <-> the same for every pair of a batch
  Context.find_homography / homography_batch / batch_homography   homography RANSAC and the H-or-E model choice (beyond the reference)
  Context.homography_pose / homography_pose_batch / batch_homography_pose   (R, t / d, n) of a pair's homography, both survivors of the vote
  Context.homography_polish / homography_polish_batch / batch_homography_polish   the homography refined over its inliers, between the two above
  Context.pnp_ransac / pnp_batch / batch_pnp   the pose of a frame against map points: P3P RANSAC + Gauss-Newton refinement (beyond the reference)
  Context.essential_batch                             <-> essential RANSAC + recoverPose on rows that already sit in device memory
  Context.essential_refine / essential_refine_batch / batch_essential_refine   Gauss-Newton refinement of the two-view pose (beyond the reference)
  Context.essential_polish / essential_polish_batch / batch_essential_polish   the refinement with its inlier set re-selected (beyond the reference)
  Context.batch_triangulate_from                      batch_triangulate from caller pose records and mask rows (the polished ones)
  Context.filter_keypoints (_batch, batch_...)        <-> VISystem::FilterKeypoints  (src/VISystem.cpp:542-610)

There is NO CPU fallback: if the HIP library is missing, importing this module raises.
"""
import ctypes as C
import os

import numpy as np

# PyTorch (plumbing for device memory / streams / torch.distributed in tests and bench.py) bundles its
# own libamdhip64.so.7.  Two HIP runtimes in one process cannot both own the GPU, so when torch is
# installed it is imported FIRST: the loader then resolves this library's libamdhip64.so.7 dependency
# to the copy that is already mapped.  The library itself has no torch dependency.
try:  # pragma: no cover
    import torch  # noqa: F401
except ImportError:  # pragma: no cover
    torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))
# VISLAM_HIP_LIB: another build of the same library (A/B measurements); there is no fallback either way
LIB_PATH = os.environ.get("VISLAM_HIP_LIB") or os.path.join(_HERE, "..", "lib", "libvislam_hip.so")


class VisError(RuntimeError):
    def __init__(self, code, where, detail=""):
        self.code = code
        super().__init__(f"{where}: error {code} ({_strerror(code)}) {detail}")


class Params(C.Structure):
    _fields_ = [
        ("nfeatures", C.c_int32), ("nlevels", C.c_int32), ("scale_factor", C.c_float),
        ("edge_threshold", C.c_int32), ("patch_size", C.c_int32), ("fast_threshold", C.c_int32),
        ("ratio", C.c_float), ("n_cells", C.c_int32), ("w_size", C.c_int32), ("h_size", C.c_int32),
        ("sym_mode", C.c_int32),
        ("ransac_prob", C.c_double), ("ransac_threshold", C.c_double),
        ("ransac_max_iters", C.c_int32), ("ransac_adaptive", C.c_int32), ("ransac_seed", C.c_uint64),
        ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
        ("f2f_iters", C.c_int32), ("f2f_threshold", C.c_double),
        ("pose_input", C.c_int32), ("keypoint_capacity", C.c_int32),
        ("keyframe_min_points", C.c_int32),
    ]

    def copy(self):
        p = Params()
        C.memmove(C.byref(p), C.byref(self), C.sizeof(Params))
        return p


class Se3f(C.Structure):
    """Sophus::SE3f storage order: unit quaternion (x, y, z, w) + translation"""
    _fields_ = [("qx", C.c_float), ("qy", C.c_float), ("qz", C.c_float), ("qw", C.c_float),
                ("tx", C.c_float), ("ty", C.c_float), ("tz", C.c_float)]

    def as_array(self):
        return np.array([self.qx, self.qy, self.qz, self.qw, self.tx, self.ty, self.tz], np.float32)


class AlignParams(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("first_level", C.c_int32), ("last_level", C.c_int32), ("max_iterations", C.c_int32),
                ("epsilon", C.c_float), ("z_factor", C.c_float)]


class AlignResult(C.Structure):
    _fields_ = [("pose", Se3f), ("matrix", C.c_float * 16), ("error", C.c_float * 5), ("initial_error", C.c_float),
                ("iterations", C.c_int32 * 5), ("n_residuals", C.c_int32 * 5)]


class AlignWeights(C.Structure):
    """vis_align_weights: the weighting of the alignment's Gauss-Newton step (vis_default_align_weights: W_IDENTITY, 4.6851, 1.4826)"""
    _fields_ = [("mode", C.c_int32), ("tukey_b", C.c_float), ("mad_scale", C.c_float), ("reserved_", C.c_int32)]


assert C.sizeof(AlignWeights) == 16
W_IDENTITY, W_TUKEY, W_TUKEY_SIGNED = 0, 1, 2


class TrackResult(C.Structure):
    """vis_track_result: final_poseCam after a frame (VISystem::Track) and the pair whose residual was composed for it"""
    _fields_ = [("pose", Se3f), ("composed", C.c_int32)]


assert C.sizeof(TrackResult) == 32


class PoseResult(C.Structure):
    _fields_ = [("E", C.c_double * 9), ("R", C.c_double * 9), ("t", C.c_double * 3), ("n_inliers", C.c_int32), ("n_pose_good", C.c_int32),
                ("iters_run", C.c_int32), ("n_points", C.c_int32), ("n_models", C.c_int32), ("undecided_max", C.c_int32)]


POSE_RESULT_DTYPE = np.dtype([("E", "<f8", (9,)), ("R", "<f8", (9,)), ("t", "<f8", (3,)), ("n_inliers", "<i4"), ("n_pose_good", "<i4"),
                              ("iters_run", "<i4"), ("n_points", "<i4"), ("n_models", "<i4"), ("undecided_max", "<i4")])
assert POSE_RESULT_DTYPE.itemsize == C.sizeof(PoseResult) == 192


class TriParams(C.Structure):
    """vis_tri_params: the thresholds of the map-point flags (vis_default_tri_params: 2.0 px, 0 px, 0)"""
    _fields_ = [("max_reproj_px", C.c_float), ("min_parallax_px", C.c_float), ("inliers_only", C.c_int32), ("reserved_", C.c_int32)]


class MapPoint(C.Structure):
    """vis_map_point: the triangulated point (first camera's frame, units of the baseline) and its two per-point errors"""
    _fields_ = [("X", C.c_double * 3), ("reproj_px", C.c_float), ("parallax_px", C.c_float)]


class TriSummary(C.Structure):
    _fields_ = [("n_points", C.c_int32), ("n_front", C.c_int32), ("n_kept", C.c_int32), ("mean_parallax_px", C.c_float)]


MAP_POINT_DTYPE = np.dtype([("X", "<f8", (3,)), ("reproj_px", "<f4"), ("parallax_px", "<f4")])
TRI_SUMMARY_DTYPE = np.dtype([("n_points", "<i4"), ("n_front", "<i4"), ("n_kept", "<i4"), ("mean_parallax_px", "<f4")])
assert C.sizeof(TriParams) == 16 and MAP_POINT_DTYPE.itemsize == C.sizeof(MapPoint) == 32 and TRI_SUMMARY_DTYPE.itemsize == C.sizeof(TriSummary) == 16
MP_INLIER, MP_FRONT, MP_REPROJ_OK, MP_PARALLAX_OK, MP_KEPT = 1, 2, 4, 8, 16


class F2fResult(C.Structure):
    """vis_f2f_result: the translation F2FRansac gives one pair (scale * direction, sign-fixed) and how it was won"""
    _fields_ = [("t", C.c_float * 3), ("count_max", C.c_int32), ("n_points", C.c_int32), ("best_iter", C.c_int32),
                ("n_degenerate", C.c_int32), ("flipped", C.c_int32)]


F2F_RESULT_DTYPE = np.dtype([("t", "<f4", (3,)), ("count_max", "<i4"), ("n_points", "<i4"), ("best_iter", "<i4"), ("n_degenerate", "<i4"),
                             ("flipped", "<i4")])
assert F2F_RESULT_DTYPE.itemsize == C.sizeof(F2fResult) == 32
F2F_TILE = 512                                    # VIS_F2F_TILE: correspondences per LDS tile of the batched F2FRansac kernel


class HomographyParams(C.Structure):
    """vis_homography_params: the knobs of the homography RANSAC and of the H-or-E decision (vis_default_homography_params: 200, 8, 5.991,
    3.841, 1.0, 0.40)"""
    _fields_ = [("iters", C.c_int32), ("min_inliers", C.c_int32), ("chi2_h", C.c_double), ("chi2_e", C.c_double), ("sigma_px", C.c_double),
                ("h_ratio", C.c_double)]


class HomographyResult(C.Structure):
    """vis_homography_result: the winning homography of one pair (normalised coordinates, unit norm, det >= 0), both models' scores and the choice"""
    _fields_ = [("H", C.c_double * 9), ("score_h", C.c_double), ("score_e", C.c_double), ("n_inliers", C.c_int32), ("n_points", C.c_int32),
                ("best_iter", C.c_int32), ("n_degenerate", C.c_int32), ("n_inliers_e", C.c_int32), ("model", C.c_int32)]


HOMOGRAPHY_RESULT_DTYPE = np.dtype([("H", "<f8", (9,)), ("score_h", "<f8"), ("score_e", "<f8"), ("n_inliers", "<i4"), ("n_points", "<i4"),
                                    ("best_iter", "<i4"), ("n_degenerate", "<i4"), ("n_inliers_e", "<i4"), ("model", "<i4")])
assert C.sizeof(HomographyParams) == 40 and HOMOGRAPHY_RESULT_DTYPE.itemsize == C.sizeof(HomographyResult) == 112
H_TILE = 512                                      # VIS_H_TILE: correspondences per LDS tile of the homography kernel
MODEL_NONE, MODEL_HOMOGRAPHY, MODEL_ESSENTIAL = 0, 1, 2
MODEL_NAMES = ("none", "homography", "essential")


class HposeParams(C.Structure):
    """vis_hpose_params: the knobs of the homography pose (vis_default_hpose_params: 0.05, cos 1 deg, 0.75, 0.9, 0.5, 8)"""
    _fields_ = [("min_t_over_d", C.c_double), ("max_cos_parallax", C.c_double), ("ambiguity_ratio", C.c_double), ("good_share", C.c_double),
                ("parallax_share", C.c_double), ("min_good", C.c_int32), ("reserved_", C.c_int32)]


class HposeResult(C.Structure):
    """vis_hpose_result: the chosen and the second candidate (R, t / d, n) of one pair's homography, the votes and the flags"""
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("n", C.c_double * 3), ("R2", C.c_double * 9), ("t2", C.c_double * 3),
                ("n2", C.c_double * 3), ("sv", C.c_double * 3), ("t_norm", C.c_double), ("n_good", C.c_int32 * 4), ("kind", C.c_int32),
                ("flags", C.c_int32), ("solution", C.c_int32), ("second", C.c_int32), ("n_tested", C.c_int32), ("n_parallax", C.c_int32),
                ("n_points", C.c_int32), ("reserved_", C.c_int32)]


HPOSE_RESULT_DTYPE = np.dtype([("R", "<f8", (9,)), ("t", "<f8", (3,)), ("n", "<f8", (3,)), ("R2", "<f8", (9,)), ("t2", "<f8", (3,)), ("n2", "<f8", (3,)),
                               ("sv", "<f8", (3,)), ("t_norm", "<f8"), ("n_good", "<i4", (4,)), ("kind", "<i4"), ("flags", "<i4"), ("solution", "<i4"),
                               ("second", "<i4"), ("n_tested", "<i4"), ("n_parallax", "<i4"), ("n_points", "<i4"), ("reserved_", "<i4")])
assert C.sizeof(HposeParams) == 48 and HPOSE_RESULT_DTYPE.itemsize == C.sizeof(HposeResult) == 320
HP_NONE, HP_ROTATION, HP_PLANE = 0, 1, 2
HPF_AMBIGUOUS, HPF_HINTED, HPF_FEW, HPF_LOW_PARALLAX = 1, 2, 4, 8
HP_KIND_NAMES = ("none", "rotation", "plane")


class PnpParams(C.Structure):
    """vis_pnp_params: the knobs of the P3P RANSAC and its refinement (vis_default_pnp_params: 200, 8, 2.0, 5)"""
    _fields_ = [("iters", C.c_int32), ("min_inliers", C.c_int32), ("threshold_px", C.c_double), ("refine_iters", C.c_int32), ("reserved_", C.c_int32)]


class PnpResult(C.Structure):
    """vis_pnp_result: the reported pose (x_cam = R X + t), the winning P3P pose, the refinement's costs and the counts of one problem"""
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("R_ransac", C.c_double * 9), ("t_ransac", C.c_double * 3), ("cost0", C.c_double),
                ("cost1", C.c_double), ("n_inliers", C.c_int32), ("n_points", C.c_int32), ("best_iter", C.c_int32), ("best_root", C.c_int32),
                ("n_degenerate", C.c_int32), ("n_solutions", C.c_int32), ("n_inliers_refined", C.c_int32), ("flags", C.c_int32)]


PNP_RESULT_DTYPE = np.dtype([("R", "<f8", (9,)), ("t", "<f8", (3,)), ("R_ransac", "<f8", (9,)), ("t_ransac", "<f8", (3,)), ("cost0", "<f8"),
                             ("cost1", "<f8"), ("n_inliers", "<i4"), ("n_points", "<i4"), ("best_iter", "<i4"), ("best_root", "<i4"),
                             ("n_degenerate", "<i4"), ("n_solutions", "<i4"), ("n_inliers_refined", "<i4"), ("flags", "<i4")])
assert C.sizeof(PnpParams) == 24 and PNP_RESULT_DTYPE.itemsize == C.sizeof(PnpResult) == 240


class PnpLink(C.Structure):
    """vis_pnp_link: what vis_batch_pnp joined for one frame and the relative motion keyframe -> frame in units of the keyframe's own baseline"""
    _fields_ = [("R_rel", C.c_double * 9), ("t_rel", C.c_double * 3), ("scale", C.c_double), ("n_linked", C.c_int32), ("q", C.c_int32),
                ("p", C.c_int32), ("flags", C.c_int32)]


PNP_LINK_DTYPE = np.dtype([("R_rel", "<f8", (9,)), ("t_rel", "<f8", (3,)), ("scale", "<f8"), ("n_linked", "<i4"), ("q", "<i4"), ("p", "<i4"),
                           ("flags", "<i4")])
assert PNP_LINK_DTYPE.itemsize == C.sizeof(PnpLink) == 120
PNPL_NO_MAP = 1
PNP_TILE = 512                                    # VIS_PNP_TILE: points per LDS tile of the PnP kernel
PNP_REFINED, PNP_REFINE_REJECTED, PNP_FEW = 1, 2, 4


class EssentialRefineParams(C.Structure):
    """vis_eref_params: the knobs of the two-view refinement (vis_default_eref_params: 5, 8, 1.0)"""
    _fields_ = [("refine_iters", C.c_int32), ("min_inliers", C.c_int32), ("threshold_px", C.c_double)]


class EssentialRefineResult(C.Structure):
    """vis_eref_result: the reported pose (|t| = 1), its E = [t]x R, the costs of the start and of the reported iterate, and the counts"""
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("E", C.c_double * 9), ("cost0", C.c_double), ("cost1", C.c_double),
                ("n_used", C.c_int32), ("n_points", C.c_int32), ("n_inliers0", C.c_int32), ("n_inliers_refined", C.c_int32),
                ("best_step", C.c_int32), ("steps_run", C.c_int32), ("flags", C.c_int32), ("reserved_", C.c_int32)]


EREF_RESULT_DTYPE = np.dtype([("R", "<f8", (9,)), ("t", "<f8", (3,)), ("E", "<f8", (9,)), ("cost0", "<f8"), ("cost1", "<f8"), ("n_used", "<i4"),
                              ("n_points", "<i4"), ("n_inliers0", "<i4"), ("n_inliers_refined", "<i4"), ("best_step", "<i4"), ("steps_run", "<i4"),
                              ("flags", "<i4"), ("reserved_", "<i4")])
assert C.sizeof(EssentialRefineParams) == 16 and EREF_RESULT_DTYPE.itemsize == C.sizeof(EssentialRefineResult) == 216
ER_REFINED, ER_REJECTED, ER_FEW, ER_NO_POSE = 1, 2, 4, 8


class EssentialPolishParams(C.Structure):
    """vis_epolish_params: the knobs of the two-view polish (vis_default_epolish_params: 3, 5, 8, 2.0)"""
    _fields_ = [("rounds", C.c_int32), ("refine_iters", C.c_int32), ("min_inliers", C.c_int32), ("reserved_", C.c_int32), ("select_px", C.c_double),
                ("reserved2_", C.c_int32 * 2)]


class EssentialPolishResult(C.Structure):
    """vis_epolish_result: the reported pose (|t| = 1), its E = [t]x R, the start's cost, the last round's costs, the sets' sizes and the counts"""
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("E", C.c_double * 9), ("cost_first", C.c_double), ("cost0", C.c_double),
                ("cost1", C.c_double), ("n_points", C.c_int32), ("n_set_first", C.c_int32), ("n_set_last", C.c_int32), ("n_changed", C.c_int32),
                ("rounds_run", C.c_int32), ("steps_run", C.c_int32), ("best_step", C.c_int32), ("flags", C.c_int32)]


EPOLISH_RESULT_DTYPE = np.dtype([("R", "<f8", (9,)), ("t", "<f8", (3,)), ("E", "<f8", (9,)), ("cost_first", "<f8"), ("cost0", "<f8"), ("cost1", "<f8"),
                                 ("n_points", "<i4"), ("n_set_first", "<i4"), ("n_set_last", "<i4"), ("n_changed", "<i4"), ("rounds_run", "<i4"),
                                 ("steps_run", "<i4"), ("best_step", "<i4"), ("flags", "<i4")])
assert C.sizeof(EssentialPolishParams) == 32 and EPOLISH_RESULT_DTYPE.itemsize == C.sizeof(EssentialPolishResult) == 224
EP_POLISHED, EP_REJECTED, EP_FEW, EP_NO_POSE, EP_SHRANK = 1, 2, 4, 8, 16


class HomographyPolishParams(C.Structure):
    """vis_hpolish_params: the knobs of the homography polish (vis_default_hpolish_params: 3, 5, 8, 5.991, 1.0)"""
    _fields_ = [("rounds", C.c_int32), ("refine_iters", C.c_int32), ("min_inliers", C.c_int32), ("reserved_", C.c_int32),
                ("select_chi2", C.c_double), ("sigma_px", C.c_double)]


class HomographyPolishResult(C.Structure):
    """vis_hpolish_result: the reported H (unit norm, det >= 0), the start's cost, the last round's costs, the sets' sizes and the counts"""
    _fields_ = [("H", C.c_double * 9), ("cost_first", C.c_double), ("cost0", C.c_double), ("cost1", C.c_double), ("n_points", C.c_int32),
                ("n_set_first", C.c_int32), ("n_set_last", C.c_int32), ("n_changed", C.c_int32), ("rounds_run", C.c_int32),
                ("steps_run", C.c_int32), ("best_step", C.c_int32), ("flags", C.c_int32)]


HPOLISH_RESULT_DTYPE = np.dtype([("H", "<f8", (9,)), ("cost_first", "<f8"), ("cost0", "<f8"), ("cost1", "<f8"), ("n_points", "<i4"),
                                 ("n_set_first", "<i4"), ("n_set_last", "<i4"), ("n_changed", "<i4"), ("rounds_run", "<i4"), ("steps_run", "<i4"),
                                 ("best_step", "<i4"), ("flags", "<i4")])
assert C.sizeof(HomographyPolishParams) == 32 and HPOLISH_RESULT_DTYPE.itemsize == C.sizeof(HomographyPolishResult) == 128
HPOL_POLISHED, HPOL_REJECTED, HPOL_FEW, HPOL_NO_MODEL, HPOL_SHRANK = 1, 2, 4, 8, 16


class KltParams(C.Structure):
    """vis_klt_params: the knobs of the pyramidal KLT tracker (vis_default_klt_params: 7, 3, 0, 10, 0.01, 0.1, 0, 0, 3)"""
    _fields_ = [("win_radius", C.c_int32), ("first_level", C.c_int32), ("last_level", C.c_int32), ("max_iters", C.c_int32),
                ("epsilon", C.c_double), ("min_eig", C.c_double), ("max_err", C.c_double), ("fb_max_px", C.c_double),
                ("scharr_scale", C.c_int32), ("reserved_", C.c_int32)]


KLT_POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("fb", "<f4"), ("min_eig", "<f4"), ("sad", "<i4"), ("flags", "<i4"), ("iters", "<u2"),
                            ("levels", "u1"), ("pad_", "u1", (5,))])
KLT_PAIR_DTYPE = np.dtype([("n_points", "<i4"), ("n_tracked", "<i4"), ("n_oob", "<i4"), ("n_flat", "<i4"), ("n_err", "<i4"), ("n_fb", "<i4"),
                           ("n_invalid", "<i4"), ("flags", "<i4")])
assert C.sizeof(KltParams) == 56 and KLT_POINT_DTYPE.itemsize == 32 and KLT_PAIR_DTYPE.itemsize == 32
KLT_TRACKED, KLT_OOB, KLT_FLAT, KLT_ERR, KLT_FB, KLT_INVALID = 1, 2, 4, 8, 16, 32
KLT_NO_PAIR = 1


class FtrackTriParams(C.Structure):
    """vis_ftrack_tri_params: the knobs of the N-view triangulation of feature tracks (vis_default_ftrack_tri_params: 16, 2, 5, 2.0, cos 1 deg)"""
    _fields_ = [("max_views", C.c_int32), ("min_views", C.c_int32), ("gn_iters", C.c_int32), ("reserved_", C.c_int32), ("max_reproj_px", C.c_double),
                ("max_parallax_cos", C.c_double)]


FTRACK_OBS_DTYPE = np.dtype([("birth_seq", "<i4"), ("birth_kp", "<i4"), ("len", "<i4"), ("prev_kp", "<i4")])
FTRACK_FRAME_DTYPE = np.dtype([("seq", "<i4"), ("n_keypoints", "<i4"), ("n_continued", "<i4"), ("n_started", "<i4"), ("n_ended", "<i4"),
                               ("max_len", "<i4"), ("sum_len", "<i4"), ("flags", "<i4")])
FTRACK_POINT_DTYPE = np.dtype([("X", "<f8", (3,)), ("rms_reproj_px", "<f4"), ("parallax_cos", "<f4"), ("n_views", "<i4"), ("flags", "<i4")])
FTRACK_TRI_SUMMARY_DTYPE = np.dtype([("n_ends", "<i4"), ("n_points", "<i4"), ("n_kept", "<i4"), ("n_front", "<i4"), ("n_reproj_ok", "<i4"),
                                     ("n_parallax_ok", "<i4"), ("n_few", "<i4"), ("n_singular", "<i4")])
assert FTRACK_OBS_DTYPE.itemsize == 16 and FTRACK_FRAME_DTYPE.itemsize == 32 and FTRACK_POINT_DTYPE.itemsize == 40
assert FTRACK_TRI_SUMMARY_DTYPE.itemsize == 32 and C.sizeof(FtrackTriParams) == 32


class BaParams(C.Structure):
    """vis_ba_params: the knobs of the windowed bundle adjustment (vis_default_ba_params: 8, 2, 12, 10, 5, 2.4477, 16.0, 1e-4)"""
    _fields_ = [("stride", C.c_int32), ("min_views", C.c_int32), ("min_points", C.c_int32), ("lm_iters", C.c_int32), ("tri_gn_iters", C.c_int32),
                ("reserved_", C.c_int32), ("huber_px", C.c_double), ("init_reproj_px", C.c_double), ("lambda0", C.c_double)]


BA_WINDOW_DTYPE = np.dtype([("first", "<i4"), ("last", "<i4"), ("anchor", "<i4"), ("n_free", "<i4"), ("n_points", "<i4"), ("n_obs", "<i4"),
                            ("n_lin", "<i4"), ("n_accepted", "<i4"), ("n_rejected", "<i4"), ("flags", "<i4"), ("reserved_", "<i4", (2,)),
                            ("cost0", "<f8"), ("cost1", "<f8"), ("lambda_", "<f8"), ("scale", "<f8")])
BA_POINT_DTYPE = np.dtype([("X", "<f8", (3,)), ("rms0_px", "<f4"), ("rms1_px", "<f4"), ("n_views", "<i4"), ("flags", "<i4")])
assert BA_WINDOW_DTYPE.itemsize == 80 and BA_POINT_DTYPE.itemsize == 40 and C.sizeof(BaParams) == 48
BA_REFINED, BA_FEW, BA_RESTART, BA_NO_SCALE = 1, 2, 4, 8
BAP_USED, BAP_INIT_REJECTED, BAP_FEW = 1, 2, 4


def ba_windows(n, stride):
    """the number of vis_ba_window records vis_ba_rows / vis_batch_ba write for n frames"""
    return (n - 1 + stride - 1) // stride if n > 1 else 0


class LoopParams(C.Structure):
    """vis_loop_params: the knobs of the loop-candidate scorer (vis_default_loop_params: 0.8f, SYM_INTENDED, 30, 4, 30)"""
    _fields_ = [("ratio", C.c_float), ("sym_mode", C.c_int32), ("min_gap", C.c_int32), ("topk", C.c_int32), ("min_score", C.c_int32),
                ("reserved_", C.c_int32)]


class KfDbInfo(C.Structure):
    """vis_kfdb_info_t"""
    _fields_ = [("entry_cap", C.c_int32), ("kp_cap", C.c_int32), ("head", C.c_int32), ("reserved_", C.c_int32), ("total_added", C.c_int64)]


LOOP_CAND_DTYPE = np.dtype([("id", "<i4"), ("slot", "<i4"), ("score", "<i4"), ("n_keypoints", "<i4")])
LOOP_QUERY_DTYPE = np.dtype([("id", "<i4"), ("n_keypoints", "<i4"), ("n_scored", "<i4"), ("n_cand", "<i4"), ("best_score", "<i4"), ("flags", "<i4"),
                             ("reserved_", "<i4", (2,))])
assert LOOP_CAND_DTYPE.itemsize == 16 and LOOP_QUERY_DTYPE.itemsize == 32 and C.sizeof(LoopParams) == 24 and C.sizeof(KfDbInfo) == 24
LOOP_SKIPPED = 1


FT_NO_PAIR, FT_NO_CARRY = 1, 2
FT_SYM, FT_GOOD = 0, 1
FTP_FRONT, FTP_REPROJ_OK, FTP_PARALLAX_OK, FTP_KEPT, FTP_FEW, FTP_SINGULAR = 1, 2, 4, 8, 16, 32


class ScaleLinkParams(C.Structure):
    """vis_scale_link_params: the knobs of the scale links (vis_default_scale_link_params: VIS_MP_KEPT, 8, 1.0, 1/64, 64)"""
    _fields_ = [("require", C.c_int32), ("min_shared", C.c_int32), ("max_rel_spread", C.c_double), ("min_scale", C.c_double), ("max_scale", C.c_double)]


class TrajPose(C.Structure):
    """vis_traj_pose as a host structure (vis_batch_trajectory_init)"""
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("sigma", C.c_double), ("segment_seq", C.c_int32), ("epoch_seq", C.c_int32),
                ("hops", C.c_int32), ("unit_edges", C.c_int32), ("parent", C.c_int32), ("flags", C.c_int32)]


SCALE_LINK_DTYPE = np.dtype([("scale", "<f8"), ("q25", "<f8"), ("q75", "<f8"), ("n_shared", "<i4"), ("q", "<i4"), ("flags", "<i4"), ("reserved_", "<i4")])
TRAJ_POSE_DTYPE = np.dtype([("R", "<f8", (9,)), ("t", "<f8", (3,)), ("sigma", "<f8"), ("segment_seq", "<i4"), ("epoch_seq", "<i4"), ("hops", "<i4"),
                            ("unit_edges", "<i4"), ("parent", "<i4"), ("flags", "<i4")])
assert SCALE_LINK_DTYPE.itemsize == 40 and TRAJ_POSE_DTYPE.itemsize == 128 == C.sizeof(TrajPose) and C.sizeof(ScaleLinkParams) == 32
SL_OK, SL_NO_PAIR, SL_NO_DEPTH, SL_FEW, SL_SPREAD, SL_RANGE = 0, 1, 2, 4, 8, 16
TJ_ROOT, TJ_NO_POSE, TJ_NO_CARRY, TJ_NOT_SAVED, TJ_UNIT_EDGE, TJ_OVERFLOW = 1, 2, 4, 8, 16, 32
TJ_MAX_FRAMES = 1024


class ImuParams(C.Structure):
    """vis_imu_params: biases, the IMU-to-camera rotation (row-major) and the two flagging bounds (vis_default_imu_params: 0, identity, 0.05 s, 1 rad)"""
    _fields_ = [("bg", C.c_double * 3), ("ba", C.c_double * 3), ("r_ic", C.c_double * 9), ("max_gap_s", C.c_double), ("max_angle", C.c_double)]


class ImuSample(C.Structure):
    """vis_imu_sample: t (s), w (rad/s), a (m/s^2)"""
    _fields_ = [("t", C.c_double), ("w", C.c_double * 3), ("a", C.c_double * 3)]


class ImuDelta(C.Structure):
    """vis_imu_delta as a host structure (vis_imu_preintegrate)"""
    _fields_ = [("R", C.c_double * 9), ("v", C.c_double * 3), ("p", C.c_double * 3), ("dt", C.c_double), ("JRg", C.c_double * 9),
                ("n_steps", C.c_int32), ("flags", C.c_int32), ("q", C.c_int32), ("reserved_", C.c_int32)]


class ImuCarry(C.Structure):
    """vis_imu_carry as a host structure (vis_batch_imu_init)"""
    _fields_ = [("t_last", C.c_double), ("open", ImuDelta), ("valid", C.c_int32), ("reserved_", C.c_int32)]


IMU_SAMPLE_DTYPE = np.dtype([("t", "<f8"), ("w", "<f8", (3,)), ("a", "<f8", (3,))])
IMU_DELTA_DTYPE = np.dtype([("R", "<f8", (9,)), ("v", "<f8", (3,)), ("p", "<f8", (3,)), ("dt", "<f8"), ("JRg", "<f8", (9,)), ("n_steps", "<i4"),
                            ("flags", "<i4"), ("q", "<i4"), ("reserved_", "<i4")])
IMU_CARRY_DTYPE = np.dtype([("t_last", "<f8"), ("open", IMU_DELTA_DTYPE), ("valid", "<i4"), ("reserved_", "<i4")])
assert IMU_SAMPLE_DTYPE.itemsize == 56 == C.sizeof(ImuSample) and IMU_DELTA_DTYPE.itemsize == 216 == C.sizeof(ImuDelta)
assert IMU_CARRY_DTYPE.itemsize == 232 == C.sizeof(ImuCarry) and C.sizeof(ImuParams) == 136
IMU_OK, IMU_NO_PAIR, IMU_NO_CARRY, IMU_NO_START, IMU_EMPTY, IMU_EXTRAPOLATED, IMU_GAP, IMU_FAST, IMU_ORDER, IMU_NONFINITE = 0, 1, 2, 4, 8, 16, 32, 64, 128, 256
IMU_CARRY_TIME, IMU_CARRY_OPEN = 1, 2
IMU_MAX_FRAMES = 1024


class ImuBiasJac(C.Structure):
    """vis_imu_bias_jac: dv / dbg, dv / dba, dp / dbg, dp / dba of a delta (3 x 3 row-major), IMU_JAC_* flags, the delta's q"""
    _fields_ = [("Jvg", C.c_double * 9), ("Jva", C.c_double * 9), ("Jpg", C.c_double * 9), ("Jpa", C.c_double * 9), ("flags", C.c_int32), ("q", C.c_int32)]


class ImuJacCarry(C.Structure):
    """vis_imu_jac_carry as a host structure (vis_batch_imu_jac_init): vis_imu_carry and the Jacobians of its open delta"""
    _fields_ = [("carry", ImuCarry), ("open_jac", ImuBiasJac)]


IMU_BIAS_JAC_DTYPE = np.dtype([("Jvg", "<f8", (9,)), ("Jva", "<f8", (9,)), ("Jpg", "<f8", (9,)), ("Jpa", "<f8", (9,)), ("flags", "<i4"), ("q", "<i4")])
IMU_JAC_CARRY_DTYPE = np.dtype([("carry", IMU_CARRY_DTYPE), ("open_jac", IMU_BIAS_JAC_DTYPE)])
assert IMU_BIAS_JAC_DTYPE.itemsize == 296 == C.sizeof(ImuBiasJac) and IMU_JAC_CARRY_DTYPE.itemsize == 528 == C.sizeof(ImuJacCarry)
IMU_JAC_OK, IMU_JAC_NONFINITE = 0, 1
IMC_OK, IMC_UNUSABLE, IMC_JAC, IMC_BIAS, IMC_ANGLE, IMC_NONFINITE = 0, 1, 2, 4, 8, 16


class ImuNoise(C.Structure):
    """vis_imu_noise (vis_default_imu_noise: 1.6968e-4 rad/s/sqrt(Hz), 2.0e-3 m/s^2/sqrt(Hz)): the continuous-time densities of the gyro and the accelerometer"""
    _fields_ = [("sigma_g", C.c_double), ("sigma_a", C.c_double)]


class ImuCov(C.Structure):
    """vis_imu_cov: the upper triangle, in row order, of the 9 x 9 covariance of (dphi, dv, dp) of a delta, IMU_COV_* flags, the delta's q"""
    _fields_ = [("S", C.c_double * 45), ("flags", C.c_int32), ("q", C.c_int32)]


class ImuCovCarry(C.Structure):
    """vis_imu_cov_carry as a host structure (vis_batch_imu_cov_init): vis_imu_carry and the covariance of its open delta"""
    _fields_ = [("carry", ImuCarry), ("open_cov", ImuCov)]


IMU_COV_DTYPE = np.dtype([("S", "<f8", (45,)), ("flags", "<i4"), ("q", "<i4")])
IMU_COV_CARRY_DTYPE = np.dtype([("carry", IMU_CARRY_DTYPE), ("open_cov", IMU_COV_DTYPE)])
assert IMU_COV_DTYPE.itemsize == 368 == C.sizeof(ImuCov) and IMU_COV_CARRY_DTYPE.itemsize == 600 == C.sizeof(ImuCovCarry) and C.sizeof(ImuNoise) == 16
IMU_COV_OK, IMU_COV_NONFINITE = 0, 1


class ImuFactorParams(C.Structure):
    """vis_imu_factor_params (vis_default_imu_factor_params: 0, 0, 0): variances added to the diagonal of the covariance by threes"""
    _fields_ = [("var_rot", C.c_double), ("var_v", C.c_double), ("var_p", C.c_double)]


IMU_FACTOR_DTYPE = np.dtype([("r", "<f8", (9,)), ("chi2", "<f8"), ("chi2_rot", "<f8"), ("flags", "<i4"), ("q", "<i4")])
assert IMU_FACTOR_DTYPE.itemsize == 96 and C.sizeof(ImuFactorParams) == 24
IMF_OK, IMF_NO_PARENT, IMF_NO_STATE, IMF_NO_ALIGN, IMF_UNUSABLE, IMF_SINGULAR, IMF_NONFINITE = 0, 1, 2, 4, 8, 16, 32


def imu_cov_matrix(rec):
    """the symmetric 9 x 9 float64 matrix of an IMU_COV_DTYPE record"""
    M = np.zeros((9, 9))
    M[np.triu_indices(9)] = np.asarray(rec["S"], np.float64)
    return M + np.triu(M, 1).T


class ViAlignParams(C.Structure):
    """vis_vi_align_params (vis_default_vi_align_params: identity, 0, 9.81, 0.1, 8, 8, 4, IMU_EMPTY | IMU_GAP)"""
    _fields_ = [("r_ic", C.c_double * 9), ("p_ci", C.c_double * 3), ("G", C.c_double), ("g_tol", C.c_double), ("min_pairs", C.c_int32),
                ("min_triples", C.c_int32), ("refine_iters", C.c_int32), ("reject", C.c_int32)]


class ViTail(C.Structure):
    """vis_vi_tail: camera centre, IMU-to-root rotation and lever term of a frame, its segment and epoch, VIT_* flags"""
    _fields_ = [("C", C.c_double * 3), ("Rw", C.c_double * 9), ("L", C.c_double * 3), ("segment_seq", C.c_int32), ("epoch_seq", C.c_int32),
                ("flags", C.c_int32), ("reserved_", C.c_int32)]


class ViCarry(C.Structure):
    """vis_vi_carry as a host structure (vis_batch_vi_align_init)"""
    _fields_ = [("gyro", C.c_double * 10), ("lin", C.c_double * 16), ("n_pairs", C.c_int32), ("n_triples", C.c_int32), ("segment_seq", C.c_int32),
                ("epoch_seq", C.c_int32), ("last", ViTail), ("parent", ViTail), ("last_delta", ImuDelta), ("valid", C.c_int32), ("reserved_", C.c_int32)]


VI_STATE_DTYPE = np.dtype([("p", "<f8", (3,)), ("v", "<f8", (3,)), ("res", "<f8"), ("flags", "<i4"), ("q", "<i4")])
VI_ALIGN_DTYPE = np.dtype([("dbg", "<f8", (3,)), ("c0", "<f8"), ("c0_call", "<f8"), ("c1", "<f8"), ("s", "<f8"), ("g", "<f8", (3,)), ("s_lin", "<f8"),
                           ("g_lin", "<f8", (3,)), ("g_lin_norm", "<f8"), ("rms", "<f8"), ("n_pairs", "<i4"), ("n_triples", "<i4"),
                           ("n_pairs_call", "<i4"), ("n_triples_call", "<i4"), ("segment_seq", "<i4"), ("epoch_seq", "<i4"), ("flags", "<i4"),
                           ("reserved_", "<i4")])
VI_TAIL_DTYPE = np.dtype([("C", "<f8", (3,)), ("Rw", "<f8", (9,)), ("L", "<f8", (3,)), ("segment_seq", "<i4"), ("epoch_seq", "<i4"), ("flags", "<i4"),
                          ("reserved_", "<i4")])
VI_CARRY_DTYPE = np.dtype([("gyro", "<f8", (10,)), ("lin", "<f8", (16,)), ("n_pairs", "<i4"), ("n_triples", "<i4"), ("segment_seq", "<i4"),
                           ("epoch_seq", "<i4"), ("last", VI_TAIL_DTYPE), ("parent", VI_TAIL_DTYPE), ("last_delta", IMU_DELTA_DTYPE), ("valid", "<i4"),
                           ("reserved_", "<i4")])
assert VI_STATE_DTYPE.itemsize == 64 and VI_ALIGN_DTYPE.itemsize == 160 and VI_TAIL_DTYPE.itemsize == 136 == C.sizeof(ViTail)
assert VI_CARRY_DTYPE.itemsize == 720 == C.sizeof(ViCarry) and C.sizeof(ViAlignParams) == 128
VIA_OK, VIA_GYRO_FEW, VIA_GYRO_SINGULAR, VIA_FEW, VIA_SINGULAR, VIA_SCALE, VIA_GRAVITY_NORM, VIA_RESTART, VIA_BAD_CARRY = 0, 1, 2, 4, 8, 16, 32, 64, 128
VIS_HAS_P, VIS_HAS_V, VIS_HAS_TRIPLE, VIS_HAS_PAIR = 1, 2, 4, 8
VIT_POSED, VIT_EDGE, VIT_DELTA = 1, 2, 4
VIC_VALID = 1
VIA_MAX_FRAMES = 1024


class ViAlignBaParams(C.Structure):
    """vis_vi_align_ba_params (vis_default_vi_align_ba_params: 2^-30, 16)"""
    _fields_ = [("pivot_rel", C.c_double), ("min_ba_triples", C.c_int32), ("reserved_", C.c_int32 * 5)]


class ViBaCarry(C.Structure):
    """vis_vi_ba_carry as a host structure (vis_batch_vi_align_ba_init): vis_vi_carry, the 32 bias sums, their count, the Jacobians of last_delta"""
    _fields_ = [("carry", ViCarry), ("ba", C.c_double * 32), ("n_ba_triples", C.c_int32), ("reserved_", C.c_int32), ("last_jac", ImuBiasJac)]


VI_ALIGN_BA_DTYPE = np.dtype([("a", VI_ALIGN_DTYPE), ("dba", "<f8", (3,)), ("s_ba", "<f8"), ("g_ba", "<f8", (3,)), ("dba_lin", "<f8", (3,)),
                              ("s_lin7", "<f8"), ("g_lin7", "<f8", (3,)), ("g_lin7_norm", "<f8"), ("rms_ba", "<f8"), ("n_ba_triples", "<i4"),
                              ("n_ba_triples_call", "<i4"), ("ba_flags", "<i4"), ("reserved_", "<i4")])
VI_BA_CARRY_DTYPE = np.dtype([("carry", VI_CARRY_DTYPE), ("ba", "<f8", (32,)), ("n_ba_triples", "<i4"), ("reserved_", "<i4"),
                              ("last_jac", IMU_BIAS_JAC_DTYPE)])
assert VI_ALIGN_BA_DTYPE.itemsize == 304 and VI_BA_CARRY_DTYPE.itemsize == 1280 == C.sizeof(ViBaCarry) and C.sizeof(ViAlignBaParams) == 32
VI_ALIGN_BA_DBA_OFFSET = VI_ALIGN_BA_DTYPE.fields["dba"][1]            # 160: d_result + this is a d_dba of imu_correct_rows / batch_imu_correct
VIAB_OK, VIAB_FEW, VIAB_UNOBSERVABLE, VIAB_SCALE, VIAB_BAD_CARRY = 0, 1, 2, 4, 8
VIAB_SUMS = 32
VIAB_PIVOT_REL = 2.0 ** -30


class Timings(C.Structure):
    _fields_ = [("ms_total", C.c_float), ("ms_pyramid", C.c_float), ("ms_fast", C.c_float),
                ("ms_select", C.c_float), ("ms_describe", C.c_float), ("ms_knn", C.c_float),
                ("ms_filter", C.c_float), ("ms_pose", C.c_float),
                ("launches_fast", C.c_int32), ("launches_total", C.c_int32), ("ms_update", C.c_float), ("reserved_", C.c_float)]


KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                           ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
DMATCH_DTYPE = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])
assert KEYPOINT_DTYPE.itemsize == 28 and DMATCH_DTYPE.itemsize == 16

SYM_REFERENCE_EFFECTIVE, SYM_INTENDED = 0, 1
STAGE_DETECT, STAGE_MATCH, STAGE_POSE, STAGE_ALL = 1, 2, 4, 7
STAGE_UPDATE, STAGE_FRAME = 8, 15          # Camera::Update's half pyramid at the head of the detect chain; FRAME = ALL | UPDATE
STAGE_GRADIENT = 16                        # Camera::computeGradient into plan-owned buffers, beside the detect chain (implies UPDATE)
KF_CARRIED, KF_NOT_SAVED, KF_FIRST = -1, -2, -3   # batch_get_keyframes(): no frame of this batch to match against
TRACK_NONE = -4                                   # TrackResult.composed: Track did not run for the frame

# every symbol include/vislam_hip.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "vis_version", "vis_strerror", "vis_device_count", "vis_create", "vis_destroy", "vis_last_error",
    "vis_default_params", "vis_set_params", "vis_get_params", "vis_set_stream", "vis_last_timings",
    "vis_level_geometry", "vis_camera_update", "vis_orb_detect_compute", "vis_bf_knn2_hamming",
    "vis_bf_knn2_hamming_host", "vis_good_matches", "vis_good_matches_host", "vis_essential_ransac",
    "vis_recover_pose", "vis_f2f_ransac", "vis_batch_plan", "vis_batch_reset", "vis_batch_run",
    "vis_batch_sync", "vis_batch_get_keypoints", "vis_batch_get_knn", "vis_batch_get_matches",
    "vis_batch_get_pose", "vis_batch_get_inlier_mask", "vis_debug_counters", "vis_device_pci_bus_id", "vis_batch_status", "vis_synth_canvas", "vis_synth_frame",
    "vis_gradient_frame_elems", "vis_half_pyramid_dims", "vis_gradient_batch", "vis_compute_gradient", "vis_patch_points",
    "vis_image_list", "vis_image_time", "vis_pgm_info", "vis_image_info", "vis_image_read",
    "vis_feeder_create", "vis_feeder_destroy", "vis_feeder_host_buffer", "vis_feeder_submit", "vis_feeder_release",
    "vis_default_align_params", "vis_estimate_pose_features", "vis_align_batch", "vis_batch_align",
    "vis_synth_frame_parallax", "vis_synth_frames_device", "vis_batch_results_async", "vis_batch_half_pyramid", "vis_batch_gradients", "vis_batch_fast_thresholds",
    "vis_se3_exp", "vis_se3_mul", "vis_se3_from_rt", "vis_se3_matrix", "vis_batch_get_keyframes",
    "vis_batch_track_init", "vis_batch_track",
    "vis_optimal_new_camera_matrix", "vis_undistort_rectify_map", "vis_rectify_create", "vis_rectify_destroy", "vis_rectify_maps",
    "vis_rectify_batch", "vis_rectify_host",
    "vis_default_tri_params", "vis_triangulate", "vis_batch_triangulate",
    "vis_f2f_batch", "vis_batch_f2f", "vis_filter_keypoints_batch", "vis_batch_filter_keypoints", "vis_filter_keypoints",
    "vis_default_homography_params", "vis_find_homography", "vis_homography_batch", "vis_batch_homography",
    "vis_default_hpose_params", "vis_homography_pose", "vis_homography_pose_batch", "vis_batch_homography_pose",
    "vis_default_hpolish_params", "vis_homography_polish", "vis_homography_polish_batch", "vis_batch_homography_polish",
    "vis_default_pnp_params", "vis_pnp_ransac", "vis_pnp_batch", "vis_batch_pnp",
    "vis_essential_batch", "vis_default_eref_params", "vis_essential_refine", "vis_essential_refine_batch", "vis_batch_essential_refine",
    "vis_default_epolish_params", "vis_essential_polish", "vis_essential_polish_batch", "vis_batch_essential_polish", "vis_batch_triangulate_from",
    "vis_default_align_weights", "vis_set_align_weights", "vis_get_align_weights",
    "vis_debug_pyramid_level",
    "vis_warp_keypoints", "vis_bf_knn2_hamming_guided", "vis_bf_knn2_hamming_guided_host", "vis_good_matches_guided", "vis_batch_run_guided",
    "vis_default_klt_params", "vis_klt_track", "vis_klt_batch", "vis_batch_klt",
    "vis_ftrack_link_rows", "vis_batch_ftrack", "vis_default_ftrack_tri_params", "vis_ftrack_triangulate_rows", "vis_batch_ftrack_triangulate",
    "vis_default_scale_link_params", "vis_scale_link_rows", "vis_batch_scale_links", "vis_trajectory_rows", "vis_batch_trajectory",
    "vis_batch_trajectory_init",
    "vis_default_imu_params", "vis_imu_preintegrate", "vis_imu_preintegrate_rows", "vis_batch_imu", "vis_batch_imu_init",
    "vis_imu_preintegrate_jac", "vis_imu_preintegrate_jac_rows", "vis_batch_imu_jac", "vis_batch_imu_jac_init", "vis_imu_correct_rows",
    "vis_batch_imu_correct",
    "vis_default_imu_noise", "vis_imu_preintegrate_cov", "vis_imu_preintegrate_cov_rows", "vis_batch_imu_cov", "vis_batch_imu_cov_init",
    "vis_default_imu_factor_params", "vis_imu_factor_rows", "vis_batch_imu_factor",
    "vis_default_vi_align_params", "vis_vi_align_rows", "vis_batch_vi_align", "vis_batch_vi_align_init",
    "vis_default_vi_align_ba_params", "vis_vi_align_ba_rows", "vis_batch_vi_align_ba", "vis_batch_vi_align_ba_init",
    "vis_default_ba_params", "vis_ba_rows", "vis_batch_ba",
    "vis_default_loop_params", "vis_kfdb_create", "vis_kfdb_destroy", "vis_kfdb_reset", "vis_kfdb_info", "vis_kfdb_get_entry", "vis_kfdb_add_rows",
    "vis_batch_kfdb_add", "vis_kfdb_query_rows", "vis_batch_kfdb_query", "vis_kfdb_match_rows", "vis_batch_kfdb_match",
]


def _load():
    path = os.path.abspath(LIB_PATH)
    if not os.path.exists(path):
        raise ImportError(f"libvislam_hip.so not built at {path}: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no CPU fallback)")
    lib = C.CDLL(path)
    lib.vis_version.restype = C.c_char_p
    lib.vis_strerror.restype = C.c_char_p
    lib.vis_strerror.argtypes = [C.c_int]
    lib.vis_last_error.restype = C.c_char_p
    lib.vis_last_error.argtypes = [C.c_void_p]
    lib.vis_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.vis_destroy.argtypes = [C.c_void_p]
    lib.vis_destroy.restype = None
    lib.vis_default_params.argtypes = [C.POINTER(Params)]
    lib.vis_default_params.restype = None
    lib.vis_set_params.argtypes = [C.c_void_p, C.POINTER(Params)]
    lib.vis_get_params.argtypes = [C.c_void_p, C.POINTER(Params)]
    lib.vis_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    lib.vis_last_timings.argtypes = [C.c_void_p, C.POINTER(Timings)]
    vp, ci, ip = C.c_void_p, C.c_int, C.POINTER(C.c_int)
    lib.vis_level_geometry.argtypes = [vp, ci, ci, vp, vp, vp, vp]
    lib.vis_camera_update.argtypes = [vp, vp, ci, ci, ci, C.POINTER(C.c_void_p)]
    lib.vis_orb_detect_compute.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp, ci, ip]
    lib.vis_bf_knn2_hamming.argtypes = [vp, ci, ci, vp, vp]
    lib.vis_bf_knn2_hamming_host.argtypes = [vp, vp, ci, vp, ci, vp, vp]
    lib.vis_good_matches.argtypes = [vp, ci, ci, vp, ci, ip, vp, ci, ip]
    lib.vis_good_matches_host.argtypes = [vp, vp, ci, vp, ci, vp, vp, vp, ci, ip, vp, ci, ip]
    lib.vis_essential_ransac.argtypes = [vp, vp, vp, ci, vp, vp, ip, ip]
    lib.vis_recover_pose.argtypes = [vp, vp, vp, vp, ci, vp, vp, ip]
    lib.vis_f2f_ransac.argtypes = [vp, vp, vp, ci, vp, vp, ci, C.c_float, vp, ip]
    lib.vis_batch_plan.argtypes = [vp, ci, ci, ci, ci]
    lib.vis_batch_reset.argtypes = [vp]
    lib.vis_batch_run.argtypes = [vp, vp, ci, ci]
    lib.vis_batch_sync.argtypes = [vp]
    lib.vis_batch_get_keypoints.argtypes = [vp, ci, vp, vp, ci, ip]
    lib.vis_batch_get_knn.argtypes = [vp, ci, vp, ci, ip, vp, ci, ip]
    lib.vis_batch_get_matches.argtypes = [vp, ci, vp, ci, ip, ip]
    lib.vis_batch_get_pose.argtypes = [vp, ci, vp, vp, vp, ip, ip, ip]
    if hasattr(lib, "vis_debug_counters"):              # (absent from older A/B builds selected with VISLAM_HIP_LIB)
        lib.vis_batch_get_inlier_mask.argtypes = [vp, ci, vp, ci, ip]
        lib.vis_debug_counters.argtypes = [vp, vp]
    lib.vis_batch_status.argtypes = [vp, ip]
    if hasattr(lib, "vis_batch_get_keyframes"):         # (absent from older A/B builds)
        lib.vis_batch_get_keyframes.argtypes = [vp, vp, ci, ip]
    if hasattr(lib, "vis_batch_track"):                 # (absent from older A/B builds)
        lib.vis_batch_track_init.argtypes = [vp, C.POINTER(Se3f)]
        lib.vis_batch_track.argtypes = [vp, C.POINTER(AlignParams), vp, ci, vp, vp, vp]
    if hasattr(lib, "vis_rectify_create"):              # (absent from older A/B builds)
        lib.vis_optimal_new_camera_matrix.argtypes = [vp, vp, ci, ci, ci, ci, vp]
        lib.vis_undistort_rectify_map.argtypes = [vp, vp, vp, ci, ci, vp, vp]
        lib.vis_rectify_create.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, C.POINTER(C.c_void_p)]
        lib.vis_rectify_destroy.argtypes = [vp]
        lib.vis_rectify_destroy.restype = None
        lib.vis_rectify_maps.argtypes = [vp, vp, vp]
        lib.vis_rectify_batch.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, vp, ci]
        lib.vis_rectify_host.argtypes = [vp, vp, ci, vp, ci]
    if hasattr(lib, "vis_triangulate"):                 # (absent from older A/B builds)
        lib.vis_default_tri_params.argtypes = [C.POINTER(TriParams)]
        lib.vis_default_tri_params.restype = None
        lib.vis_triangulate.argtypes = [vp, C.POINTER(TriParams), vp, vp, vp, vp, ci, vp, vp, vp, C.POINTER(TriSummary)]
        lib.vis_batch_triangulate.argtypes = [vp, C.POINTER(TriParams), ci, ci, vp, vp, vp]
    if hasattr(lib, "vis_batch_f2f"):                   # (absent from older A/B builds)
        cd = C.c_double
        lib.vis_f2f_batch.argtypes = [vp, ci, vp, vp, vp, ci, vp, vp, vp, vp]
        lib.vis_batch_f2f.argtypes = [vp, ci, vp, vp, vp, vp]
        lib.vis_filter_keypoints_batch.argtypes = [vp, ci, vp, vp, vp, ci, vp, vp, cd, ci, vp, vp]
        lib.vis_batch_filter_keypoints.argtypes = [vp, ci, vp, vp, cd, ci, vp, vp]
        lib.vis_filter_keypoints.argtypes = [vp, vp, vp, ci, vp, vp, cd, vp, ip]
    if hasattr(lib, "vis_batch_homography"):            # (absent from older A/B builds)
        hpp = C.POINTER(HomographyParams)
        lib.vis_default_homography_params.argtypes = [hpp]
        lib.vis_default_homography_params.restype = None
        lib.vis_find_homography.argtypes = [vp, hpp, vp, vp, ci, vp, vp, vp, vp]
        lib.vis_homography_batch.argtypes = [vp, hpp, ci, vp, vp, vp, ci, vp, vp, ci, vp, vp]
        lib.vis_batch_homography.argtypes = [vp, hpp, ci, vp, ci, vp, vp]
    if hasattr(lib, "vis_pnp_batch"):                   # (absent from older A/B builds)
        ppp = C.POINTER(PnpParams)
        lib.vis_default_pnp_params.argtypes = [ppp]
        lib.vis_default_pnp_params.restype = None
        lib.vis_pnp_ransac.argtypes = [vp, ppp, vp, vp, ci, vp, vp, vp]
        lib.vis_pnp_batch.argtypes = [vp, ppp, ci, vp, ci, vp, vp, ci, vp, ci, vp, vp]
        lib.vis_batch_pnp.argtypes = [vp, ppp, ci, vp, vp, vp, ci, ci, ci, vp, vp, vp]
    if hasattr(lib, "vis_batch_ftrack"):                # (absent from older A/B builds)
        ftp = C.POINTER(FtrackTriParams)
        lib.vis_ftrack_link_rows.argtypes = [vp, ci, vp, vp, vp, vp, ci, vp, ci, vp, ci, ci, vp, vp]
        lib.vis_batch_ftrack.argtypes = [vp, ci, ci, ci, vp, ci, ci, vp, vp]
        lib.vis_default_ftrack_tri_params.argtypes = [ftp]
        lib.vis_default_ftrack_tri_params.restype = None
        lib.vis_ftrack_triangulate_rows.argtypes = [vp, ftp, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp]
        lib.vis_batch_ftrack_triangulate.argtypes = [vp, ftp, ci, vp, ci, vp, vp, vp, vp]
    if hasattr(lib, "vis_batch_ba"):                    # (absent from older A/B builds)
        bap = C.POINTER(BaParams)
        lib.vis_default_ba_params.argtypes = [bap]
        lib.vis_default_ba_params.restype = None
        lib.vis_ba_rows.argtypes = [vp, bap, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp]
        lib.vis_batch_ba.argtypes = [vp, bap, ci, vp, ci, vp, vp, vp, vp, vp]
    if hasattr(lib, "vis_kfdb_create"):                 # (absent from older A/B builds)
        lpp = C.POINTER(LoopParams)
        lib.vis_default_loop_params.argtypes = [lpp]
        lib.vis_default_loop_params.restype = None
        lib.vis_kfdb_create.argtypes = [vp, ci, ci, C.POINTER(C.c_void_p)]
        lib.vis_kfdb_destroy.argtypes = [vp]
        lib.vis_kfdb_destroy.restype = None
        lib.vis_kfdb_reset.argtypes = [vp]
        lib.vis_kfdb_info.argtypes = [vp, C.POINTER(KfDbInfo)]
        lib.vis_kfdb_get_entry.argtypes = [vp, ci, C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp, ci]
        lib.vis_kfdb_add_rows.argtypes = [vp, ci, vp, vp, vp, ci, vp]
        lib.vis_batch_kfdb_add.argtypes = [vp, ci, ci]
        lib.vis_kfdb_query_rows.argtypes = [vp, lpp, ci, vp, vp, ci, vp, vp, vp, vp]
        lib.vis_batch_kfdb_query.argtypes = [vp, lpp, ci, ci, vp, vp, vp]
        lib.vis_kfdb_match_rows.argtypes = [vp, lpp, ci, vp, vp, vp, ci, vp, ci, ci, vp, vp, vp, vp]
        lib.vis_batch_kfdb_match.argtypes = [vp, lpp, ci, vp, ci, ci, vp, vp, vp, vp]
    if hasattr(lib, "vis_batch_trajectory"):            # (absent from older A/B builds)
        slp = C.POINTER(ScaleLinkParams)
        lib.vis_default_scale_link_params.argtypes = [slp]
        lib.vis_default_scale_link_params.restype = None
        lib.vis_scale_link_rows.argtypes = [vp, slp, ci, vp, vp, vp, ci, vp, vp, vp, ci, vp, ci, vp, vp]
        lib.vis_batch_scale_links.argtypes = [vp, slp, ci, vp, vp, ci, vp]
        lib.vis_trajectory_rows.argtypes = [vp, ci, vp, vp, vp, vp, ci, ci, vp, vp]
        lib.vis_batch_trajectory.argtypes = [vp, ci, vp, ci, vp, vp]
        lib.vis_batch_trajectory_init.argtypes = [vp, C.POINTER(TrajPose)]
    if hasattr(lib, "vis_batch_imu"):                   # (absent from older A/B builds)
        imp = C.POINTER(ImuParams)
        lib.vis_default_imu_params.argtypes = [imp]
        lib.vis_default_imu_params.restype = None
        lib.vis_imu_preintegrate.argtypes = [vp, imp, vp, ci, C.c_double, C.c_double, C.POINTER(ImuDelta), vp]
        lib.vis_imu_preintegrate_rows.argtypes = [vp, imp, ci, vp, ci, vp, vp, vp, vp, vp, vp]
        lib.vis_batch_imu.argtypes = [vp, imp, ci, vp, ci, vp, vp, vp]
        lib.vis_batch_imu_init.argtypes = [vp, C.POINTER(ImuCarry)]
    if hasattr(lib, "vis_batch_imu_jac"):               # (absent from older A/B builds)
        imp = C.POINTER(ImuParams)
        lib.vis_imu_preintegrate_jac.argtypes = [vp, imp, vp, ci, C.c_double, C.c_double, C.POINTER(ImuDelta), C.POINTER(ImuBiasJac), vp]
        lib.vis_imu_preintegrate_jac_rows.argtypes = [vp, imp, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp]
        lib.vis_batch_imu_jac.argtypes = [vp, imp, ci, vp, ci, vp, vp, vp, vp]
        lib.vis_batch_imu_jac_init.argtypes = [vp, C.POINTER(ImuJacCarry)]
        lib.vis_imu_correct_rows.argtypes = [vp, imp, ci, vp, vp, vp, vp, vp, vp, vp]
        lib.vis_batch_imu_correct.argtypes = [vp, imp, ci, vp, vp, vp, vp, vp, vp, vp]
    if hasattr(lib, "vis_batch_imu_cov"):               # (absent from older A/B builds)
        imp, inp = C.POINTER(ImuParams), C.POINTER(ImuNoise)
        lib.vis_default_imu_noise.argtypes = [inp]
        lib.vis_default_imu_noise.restype = None
        lib.vis_imu_preintegrate_cov.argtypes = [vp, imp, inp, vp, ci, C.c_double, C.c_double, C.POINTER(ImuDelta), C.POINTER(ImuCov), vp]
        lib.vis_imu_preintegrate_cov_rows.argtypes = [vp, imp, inp, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp]
        lib.vis_batch_imu_cov.argtypes = [vp, imp, inp, ci, vp, ci, vp, vp, vp, vp]
        lib.vis_batch_imu_cov_init.argtypes = [vp, C.POINTER(ImuCovCarry)]
    if hasattr(lib, "vis_batch_imu_factor"):            # (absent from older A/B builds)
        vap, ifp = C.POINTER(ViAlignParams), C.POINTER(ImuFactorParams)
        lib.vis_default_imu_factor_params.argtypes = [ifp]
        lib.vis_default_imu_factor_params.restype = None
        lib.vis_imu_factor_rows.argtypes = [vp, vap, ifp, ci, vp, vp, vp, vp, vp, vp, vp]
        lib.vis_batch_imu_factor.argtypes = [vp, vap, ifp, ci, vp, vp, vp, vp, vp, vp]
    if hasattr(lib, "vis_batch_vi_align"):              # (absent from older A/B builds)
        vap = C.POINTER(ViAlignParams)
        lib.vis_default_vi_align_params.argtypes = [vap]
        lib.vis_default_vi_align_params.restype = None
        lib.vis_vi_align_rows.argtypes = [vp, vap, ci, vp, vp, vp, vp, vp, vp, vp]
        lib.vis_batch_vi_align.argtypes = [vp, vap, ci, vp, vp, vp, vp]
        lib.vis_batch_vi_align_init.argtypes = [vp, C.POINTER(ViCarry)]
    if hasattr(lib, "vis_batch_vi_align_ba"):           # (absent from older A/B builds)
        vap, vbp = C.POINTER(ViAlignParams), C.POINTER(ViAlignBaParams)
        lib.vis_default_vi_align_ba_params.argtypes = [vbp]
        lib.vis_default_vi_align_ba_params.restype = None
        lib.vis_vi_align_ba_rows.argtypes = [vp, vap, vbp, ci, vp, vp, vp, vp, vp, vp, vp, vp]
        lib.vis_batch_vi_align_ba.argtypes = [vp, vap, vbp, ci, vp, vp, vp, vp, vp]
        lib.vis_batch_vi_align_ba_init.argtypes = [vp, C.POINTER(ViBaCarry)]
    if hasattr(lib, "vis_essential_refine_batch"):      # (absent from older A/B builds)
        epp = C.POINTER(EssentialRefineParams)
        lib.vis_default_eref_params.argtypes = [epp]
        lib.vis_default_eref_params.restype = None
        lib.vis_essential_batch.argtypes = [vp, ci, vp, vp, vp, ci, ci, vp, vp]
        lib.vis_essential_refine.argtypes = [vp, epp, vp, vp, vp, vp, ci, vp, vp]
        lib.vis_essential_refine_batch.argtypes = [vp, epp, ci, vp, vp, vp, vp, ci, ci, vp, vp]
        lib.vis_batch_essential_refine.argtypes = [vp, epp, ci, vp]
    if hasattr(lib, "vis_essential_polish_batch"):      # (absent from older A/B builds)
        eqp = C.POINTER(EssentialPolishParams)
        lib.vis_default_epolish_params.argtypes = [eqp]
        lib.vis_default_epolish_params.restype = None
        lib.vis_essential_polish.argtypes = [vp, eqp, vp, vp, vp, vp, ci, vp, vp, vp, vp]
        lib.vis_essential_polish_batch.argtypes = [vp, eqp, ci, vp, vp, vp, vp, ci, ci, vp, vp, vp, vp]
        lib.vis_batch_essential_polish.argtypes = [vp, eqp, ci, ci, vp, vp, vp]
        lib.vis_batch_triangulate_from.argtypes = [vp, C.POINTER(TriParams), ci, vp, ci, vp, ci, vp, vp, vp]
    if hasattr(lib, "vis_batch_homography_pose"):       # (absent from older A/B builds)
        hqp = C.POINTER(HposeParams)
        lib.vis_default_hpose_params.argtypes = [hqp]
        lib.vis_default_hpose_params.restype = None
        lib.vis_homography_pose.argtypes = [vp, hqp, vp, vp, vp, ci, vp, vp, vp]
        lib.vis_homography_pose_batch.argtypes = [vp, hqp, ci, vp, vp, vp, vp, ci, ci, vp, vp, vp]
        lib.vis_batch_homography_pose.argtypes = [vp, hqp, ci, vp, ci, vp, vp, vp]
    if hasattr(lib, "vis_batch_homography_polish"):     # (absent from older A/B builds)
        hlp = C.POINTER(HomographyPolishParams)
        lib.vis_default_hpolish_params.argtypes = [hlp]
        lib.vis_default_hpolish_params.restype = None
        lib.vis_homography_polish.argtypes = [vp, hlp, vp, vp, vp, ci, vp, vp, vp, vp]
        lib.vis_homography_polish_batch.argtypes = [vp, hlp, ci, vp, vp, vp, vp, ci, ci, vp, vp, vp, vp]
        lib.vis_batch_homography_polish.argtypes = [vp, hlp, ci, vp, ci, vp, ci, vp, vp, vp]
    if hasattr(lib, "vis_set_align_weights"):           # (absent from older A/B builds)
        lib.vis_default_align_weights.argtypes = [C.POINTER(AlignWeights)]
        lib.vis_default_align_weights.restype = None
        lib.vis_set_align_weights.argtypes = [vp, C.POINTER(AlignWeights)]
        lib.vis_get_align_weights.argtypes = [vp, C.POINTER(AlignWeights)]
    if hasattr(lib, "vis_debug_pyramid_level"):         # (absent from older A/B builds)
        lib.vis_debug_pyramid_level.argtypes = [vp, ci, ci, ci, vp, ci]
    if hasattr(lib, "vis_batch_run_guided"):            # (absent from older A/B builds)
        cf = C.c_float
        lib.vis_warp_keypoints.argtypes = [vp, vp, ci, vp, vp]
        lib.vis_bf_knn2_hamming_guided.argtypes = [vp, ci, ci, vp, cf, vp, vp]
        lib.vis_bf_knn2_hamming_guided_host.argtypes = [vp, vp, vp, ci, vp, vp, ci, vp, cf, vp, vp]
        lib.vis_good_matches_guided.argtypes = [vp, ci, ci, vp, cf, vp, ci, ip, vp, ci, ip]
        lib.vis_batch_run_guided.argtypes = [vp, vp, ci, ci, vp, cf]
    if hasattr(lib, "vis_batch_klt"):                   # (absent from older A/B builds)
        kpp, pv5 = C.POINTER(KltParams), C.POINTER(C.c_void_p)
        lib.vis_default_klt_params.argtypes = [kpp]
        lib.vis_default_klt_params.restype = None
        lib.vis_klt_track.argtypes = [vp, kpp, ci, ci, pv5, pv5, pv5, pv5, pv5, pv5, vp, vp, ci, vp, vp]
        lib.vis_klt_batch.argtypes = [vp, kpp, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp]
        lib.vis_batch_klt.argtypes = [vp, kpp, vp, ci, vp, ci, vp, vp, vp, vp, vp]
    lib.vis_synth_canvas.argtypes = [vp, ci, C.c_uint64]
    lib.vis_synth_frame.argtypes = [vp, ci, C.c_uint64, ci, ci, ci, vp, ci]
    lib.vis_gradient_frame_elems.argtypes = [ci, ci]
    lib.vis_gradient_frame_elems.restype = C.c_size_t
    lib.vis_half_pyramid_dims.argtypes = [ci, ci, C.c_void_p, C.c_void_p]
    lib.vis_half_pyramid_dims.restype = None
    lib.vis_gradient_batch.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp]
    lib.vis_compute_gradient.argtypes = [vp, vp, ci, ci, ci, ci, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    lib.vis_patch_points.argtypes = [vp, vp, ci, ci, C.POINTER(C.c_void_p), ip, C.POINTER(C.c_void_p), ip]
    lib.vis_image_list.argtypes = [C.c_char_p, vp, ci, ip]
    lib.vis_image_time.argtypes = [C.c_char_p]
    lib.vis_image_time.restype = C.c_long
    lib.vis_pgm_info.argtypes = [C.c_char_p, ip, ip]
    lib.vis_image_info.argtypes = [C.c_char_p, ip, ip]
    lib.vis_image_read.argtypes = [C.c_char_p, vp, ci, ci, ci]
    lib.vis_feeder_create.argtypes = [vp, ci, ci, ci, C.POINTER(C.c_void_p)]
    lib.vis_feeder_destroy.argtypes = [vp]
    lib.vis_feeder_destroy.restype = None
    lib.vis_feeder_host_buffer.argtypes = [vp, ci]
    lib.vis_feeder_host_buffer.restype = C.c_void_p
    lib.vis_feeder_submit.argtypes = [vp, ci, ci, C.POINTER(C.c_void_p)]
    lib.vis_feeder_release.argtypes = [vp, ci]
    lib.vis_synth_frame_parallax.argtypes = [vp, ci, C.c_uint64, ci, ci, ci, vp, ci]
    lib.vis_synth_frames_device.argtypes = [vp, vp, ci, C.c_uint64, ci, ci, ci, ci, ci, ci, vp]
    lib.vis_batch_results_async.argtypes = [vp, vp, vp, vp, ci]
    lib.vis_batch_half_pyramid.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    lib.vis_batch_gradients.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    lib.vis_batch_fast_thresholds.argtypes = [vp, vp, C.POINTER(C.c_int32)]
    lib.vis_se3_exp.argtypes = [vp, C.POINTER(Se3f)]; lib.vis_se3_exp.restype = None
    lib.vis_se3_mul.argtypes = [C.POINTER(Se3f), C.POINTER(Se3f), C.POINTER(Se3f)]; lib.vis_se3_mul.restype = None
    lib.vis_se3_from_rt.argtypes = [vp, vp, C.POINTER(Se3f)]; lib.vis_se3_from_rt.restype = None
    lib.vis_se3_matrix.argtypes = [C.POINTER(Se3f), vp]; lib.vis_se3_matrix.restype = None
    lib.vis_default_align_params.argtypes = [C.POINTER(AlignParams)]
    lib.vis_default_align_params.restype = None
    pv = C.POINTER(C.c_void_p)
    lib.vis_estimate_pose_features.argtypes = [vp, C.POINTER(AlignParams), ci, ci, pv, pv, pv, pv, pv, ip, C.POINTER(Se3f), C.POINTER(AlignResult)]
    lib.vis_align_batch.argtypes = [vp, C.POINTER(AlignParams), vp, ci, ci, ci, ci, vp, vp, vp, vp, vp, ci, vp, vp]
    lib.vis_batch_align.argtypes = [vp, C.POINTER(AlignParams), vp, ci, vp, vp, vp, vp, vp]
    return lib


lib = _load()


def _strerror(code):
    return lib.vis_strerror(int(code)).decode()


def version():
    return lib.vis_version().decode()


def device_pci_bus_id(device):
    """PCI address of a HIP device ("" when the library cannot tell: no device / an older A/B build)"""
    if not hasattr(lib, "vis_device_pci_bus_id"):
        return ""
    buf = C.create_string_buffer(32)
    return buf.value.decode() if lib.vis_device_pci_bus_id(int(device), buf, 32) == 0 else ""


def device_count():
    return int(lib.vis_device_count())


def default_params():
    p = Params()
    lib.vis_default_params(C.byref(p))
    return p


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def default_align_params():
    ap = AlignParams()
    lib.vis_default_align_params(C.byref(ap))
    return ap


def default_align_weights():
    aw = AlignWeights()
    lib.vis_default_align_weights(C.byref(aw))
    return aw


def default_tri_params():
    tp = TriParams()
    lib.vis_default_tri_params(C.byref(tp))
    return tp


def default_homography_params():
    hp = HomographyParams()
    lib.vis_default_homography_params(C.byref(hp))
    return hp


def default_pnp_params():
    pp = PnpParams()
    lib.vis_default_pnp_params(C.byref(pp))
    return pp


def default_imu_params():
    ip = ImuParams()
    lib.vis_default_imu_params(C.byref(ip))
    return ip


def default_imu_factor_params():
    fp = ImuFactorParams()
    lib.vis_default_imu_factor_params(C.byref(fp))
    return fp


def default_imu_noise():
    noise = ImuNoise()
    lib.vis_default_imu_noise(C.byref(noise))
    return noise


def default_vi_align_ba_params():
    bp = ViAlignBaParams()
    lib.vis_default_vi_align_ba_params(C.byref(bp))
    return bp


def default_vi_align_params():
    vp = ViAlignParams()
    lib.vis_default_vi_align_params(C.byref(vp))
    return vp


def default_scale_link_params():
    sp = ScaleLinkParams()
    lib.vis_default_scale_link_params(C.byref(sp))
    return sp


def default_loop_params():
    lp = LoopParams()
    lib.vis_default_loop_params(C.byref(lp))
    return lp


def default_ba_params():
    bp = BaParams()
    lib.vis_default_ba_params(C.byref(bp))
    return bp


def default_ftrack_tri_params():
    tp = FtrackTriParams()
    lib.vis_default_ftrack_tri_params(C.byref(tp))
    return tp


def default_eref_params():
    ep = EssentialRefineParams()
    lib.vis_default_eref_params(C.byref(ep))
    return ep


def default_epolish_params():
    ep = EssentialPolishParams()
    lib.vis_default_epolish_params(C.byref(ep))
    return ep


def default_klt_params():
    kp = KltParams()
    lib.vis_default_klt_params(C.byref(kp))
    return kp


def default_hpose_params():
    hq = HposeParams()
    lib.vis_default_hpose_params(C.byref(hq))
    return hq


def default_hpolish_params():
    hp = HomographyPolishParams()
    lib.vis_default_hpolish_params(C.byref(hp))
    return hp


def se3_exp(a):
    a = np.ascontiguousarray(a, np.float32)
    o = Se3f()
    lib.vis_se3_exp(_ptr(a), C.byref(o))
    return o


def se3_mul(a, b):
    o = Se3f()
    lib.vis_se3_mul(C.byref(a), C.byref(b), C.byref(o))
    return o


def se3_from_rt(R, t):
    R = np.ascontiguousarray(R, np.float32).reshape(9); t = np.ascontiguousarray(t, np.float32)
    o = Se3f()
    lib.vis_se3_from_rt(_ptr(R), _ptr(t), C.byref(o))
    return o


def se3_matrix(a):
    M = np.zeros(16, np.float32)
    lib.vis_se3_matrix(C.byref(a), _ptr(M))
    return M.reshape(4, 4)


# ---- synthetic stream (host-side utility of the library; integer-only, bit-reproducible) ----------
def gradient_frame_elems(w, h):
    return int(lib.vis_gradient_frame_elems(w, h))


def half_pyramid_dims(w, h):
    """(widths, heights) of Camera::Update's 5 levels: cvRound(size * 0.5) per step, round half to even (include/vislam_hip.h)"""
    lw = np.zeros(5, np.int32); lh = np.zeros(5, np.int32)
    lib.vis_half_pyramid_dims(w, h, _ptr(lw), _ptr(lh))
    return [int(x) for x in lw], [int(x) for x in lh]


# -- ImageReader (src/ImageReader.cpp): directory listing, timestamp stems, PGM / raw decode; no GPU involved --------
def image_list(directory):
    n = C.c_int(0)
    rc = lib.vis_image_list(directory.encode(), None, 0, C.byref(n))
    if rc != 0:
        raise VisError(rc, "vis_image_list")
    buf = C.create_string_buffer(max(1, n.value * 300))
    rc = lib.vis_image_list(directory.encode(), buf, len(buf), C.byref(n))
    if rc != 0:
        raise VisError(rc, "vis_image_list")
    return [x for x in buf.value.decode().split("\n") if x]


def image_time(name):
    return int(lib.vis_image_time(name.encode()))


def image_read(path, w=None, h=None):
    if w is None:
        cw, ch = C.c_int(0), C.c_int(0)
        rc = lib.vis_image_info(path.encode(), C.byref(cw), C.byref(ch))
        if rc != 0:
            raise VisError(rc, "vis_image_info")
        w, h = cw.value, ch.value
    out = np.empty((h, w), np.uint8)
    rc = lib.vis_image_read(path.encode(), _ptr(out), w, w, h)
    if rc != 0:
        raise VisError(rc, "vis_image_read")
    return out


# -- vi::CameraModel's rectification (src/CameraModel.cpp:84-105): OpenCV 3.2 restatements, parity with OpenCV unpinned --------------
def _f4(a):
    return np.ascontiguousarray(np.asarray(a, np.float32).reshape(4))


def optimal_new_camera_matrix(K, dist, in_size, out_size):
    """cv::getOptimalNewCameraMatrix(K, dist, in_size, alpha = 1, out_size): K, dist = 4 floats each ((fx, fy, cx, cy), (k1, k2, p1, p2)),
    sizes (w, h) -> K' as 4 float32"""
    K, dist, Kn = _f4(K), _f4(dist), np.zeros(4, np.float32)
    rc = lib.vis_optimal_new_camera_matrix(_ptr(K), _ptr(dist), in_size[0], in_size[1], out_size[0], out_size[1], _ptr(Kn))
    if rc:
        raise VisError(rc, "vis_optimal_new_camera_matrix")
    return Kn


def undistort_rectify_map(K, dist, Knew, out_size):
    """cv::initUndistortRectifyMap(K, dist, I, K', out_size, CV_16SC2) -> (map1 (h, w, 2) int16, map2 (h, w) uint16)"""
    w, h = out_size
    m1 = np.zeros((max(h, 1), max(w, 1), 2), np.int16); m2 = np.zeros((max(h, 1), max(w, 1)), np.uint16)
    rc = lib.vis_undistort_rectify_map(_ptr(_f4(K)), _ptr(_f4(dist)), _ptr(_f4(Knew)), w, h, _ptr(m1), _ptr(m2))
    if rc:
        raise VisError(rc, "vis_undistort_rectify_map")
    return m1, m2


class Rectify:
    """device tables of one calibration (vis_rectify_*); made by Context.rectify.  The context closes it when it closes itself (a
    vis_rectify may not outlive its context); close() before that frees the tables earlier."""

    def __init__(self, ctx, K, dist, Knew, in_size, out_size):
        self.ctx, self.in_size, self.out_size = ctx, tuple(in_size), tuple(out_size)
        self._r = C.c_void_p()
        ctx._chk(lib.vis_rectify_create(ctx._h, _ptr(_f4(K)), _ptr(_f4(dist)), _ptr(_f4(Knew)), in_size[0], in_size[1], out_size[0],
                                        out_size[1], C.byref(self._r)), "vis_rectify_create")
        ctx._rectifiers.append(self)

    def batch(self, d_in_ptr, in_stride, n, d_out_ptr, out_stride, window=None):
        """n frames (in_h x in_stride each, device) -> the window (x0, y0, w, h) of the rectified frames (h x out_stride each, device);
        window None = the whole out_w x out_h image.  Asynchronous on the context's detect stream."""
        x0, y0, w, h = window if window is not None else (0, 0) + self.out_size
        self.ctx._chk(lib.vis_rectify_batch(self._r, C.c_void_p(d_in_ptr), in_stride, n, x0, y0, w, h, C.c_void_p(d_out_ptr), out_stride),
                      "vis_rectify_batch")

    def host(self, img):
        """one host frame -> the rectified out_h x out_w frame (CameraModel::Undistort)"""
        img = np.asarray(img, np.uint8)
        if img.strides[1] != 1:
            img = np.ascontiguousarray(img)
        assert img.shape == (self.in_size[1], self.in_size[0]), img.shape
        out = np.empty((self.out_size[1], self.out_size[0]), np.uint8)
        self.ctx._chk(lib.vis_rectify_host(self._r, _ptr(img), img.strides[0], _ptr(out), out.strides[0]), "vis_rectify_host")
        return out

    def maps(self):
        """the device tables, downloaded: (map1 (h, w, 2) int16, map2 (h, w) uint16)"""
        w, h = self.out_size
        m1 = np.zeros((h, w, 2), np.int16); m2 = np.zeros((h, w), np.uint16)
        self.ctx._chk(lib.vis_rectify_maps(self._r, _ptr(m1), _ptr(m2)), "vis_rectify_maps")
        return m1, m2

    def close(self):
        if self._r:
            lib.vis_rectify_destroy(self._r)             # (while the context lives: Context.close closes its rectifiers first)
            self._r = C.c_void_p()
        if self in self.ctx._rectifiers:
            self.ctx._rectifiers.remove(self)


class KfDb:
    """a keyframe database on the device (vis_kfdb_*): a ring of entry_cap slots of kp_cap keypoints, scored by brute force against query frames;
    made by Context.kfdb.  It outlives batch_plan and batch_reset; the context closes it when it closes itself.  Every pointer is a raw DEVICE
    pointer; the rows forms are asynchronous on the context's stream, the batch forms on the pose stream (in use until batch_sync())."""

    def __init__(self, ctx, entry_cap, kp_cap):
        self.ctx, self.entry_cap, self.kp_cap = ctx, entry_cap, kp_cap
        self._d = C.c_void_p()
        ctx._chk(lib.vis_kfdb_create(ctx._h, entry_cap, kp_cap, C.byref(self._d)), "vis_kfdb_create")
        ctx._kfdbs.append(self)

    def close(self):
        if self._d:
            lib.vis_kfdb_destroy(self._d)                # (while the context lives: Context.close closes its databases first)
            self._d = C.c_void_p()
        if self in self.ctx._kfdbs:
            self.ctx._kfdbs.remove(self)

    def reset(self):
        self.ctx._chk(lib.vis_kfdb_reset(self._d), "vis_kfdb_reset")

    def info(self):
        o = KfDbInfo()
        self.ctx._chk(lib.vis_kfdb_info(self._d, C.byref(o)), "vis_kfdb_info")
        return o

    def get_entry(self, slot):
        """(id, count, (count, 2) float32 pixels) of one slot; blocks"""
        i, c = C.c_int32(0), C.c_int32(0)
        xy = np.zeros((self.kp_cap, 2), np.float32)
        self.ctx._chk(lib.vis_kfdb_get_entry(self._d, slot, C.byref(i), C.byref(c), _ptr(xy), self.kp_cap), "vis_kfdb_get_entry")
        return i.value, c.value, xy[:max(c.value, 0)].copy()

    def add_rows(self, n, d_kps_ptr, d_desc_ptr, d_nkp_ptr, row_cap, d_ids_ptr):
        v = lambda a: C.c_void_p(a) if a else None
        self.ctx._chk(lib.vis_kfdb_add_rows(self._d, n, v(d_kps_ptr), v(d_desc_ptr), v(d_nkp_ptr), row_cap, v(d_ids_ptr)), "vis_kfdb_add_rows")

    def batch_add(self, n, step=1):
        """the frames of the last batch_run on the step, id = their stream number"""
        self.ctx._chk(lib.vis_batch_kfdb_add(self._d, n, step), "vis_batch_kfdb_add")

    def query_rows(self, n, d_desc_ptr, d_nkp_ptr, row_cap, d_ids_ptr, d_scores_ptr, d_cand_ptr, d_query_ptr, lp=None):
        """scores (n x entry_cap int32, or 0), n x topk LOOP_CAND_DTYPE and n LOOP_QUERY_DTYPE records of n query rows"""
        lp = default_loop_params() if lp is None else lp
        v = lambda a: C.c_void_p(a) if a else None
        self.ctx._chk(lib.vis_kfdb_query_rows(self._d, C.byref(lp), n, v(d_desc_ptr), v(d_nkp_ptr), row_cap, v(d_ids_ptr), v(d_scores_ptr), v(d_cand_ptr),
                                              v(d_query_ptr)), "vis_kfdb_query_rows")

    def batch_query(self, n, d_scores_ptr, d_cand_ptr, d_query_ptr, step=1, lp=None):
        lp = default_loop_params() if lp is None else lp
        v = lambda a: C.c_void_p(a) if a else None
        self.ctx._chk(lib.vis_batch_kfdb_query(self._d, C.byref(lp), n, step, v(d_scores_ptr), v(d_cand_ptr), v(d_query_ptr)), "vis_batch_kfdb_query")

    def match_rows(self, n, d_kps_ptr, d_desc_ptr, d_nkp_ptr, row_cap, d_cand_ptr, cand_stride, max_pts, d_matches_ptr, d_p1_ptr, d_p2_ptr, d_npts_ptr,
                   lp=None):
        """the match list and the pixel rows (what essential_batch reads) of ONE candidate per query: the record at d_cand_ptr + 16 i cand_stride"""
        lp = default_loop_params() if lp is None else lp
        v = lambda a: C.c_void_p(a) if a else None
        self.ctx._chk(lib.vis_kfdb_match_rows(self._d, C.byref(lp), n, v(d_kps_ptr), v(d_desc_ptr), v(d_nkp_ptr), row_cap, v(d_cand_ptr), cand_stride,
                                              max_pts, v(d_matches_ptr), v(d_p1_ptr), v(d_p2_ptr), v(d_npts_ptr)), "vis_kfdb_match_rows")

    def batch_match(self, n, d_cand_ptr, cand_stride, max_pts, d_matches_ptr, d_p1_ptr, d_p2_ptr, d_npts_ptr, lp=None):
        lp = default_loop_params() if lp is None else lp
        v = lambda a: C.c_void_p(a) if a else None
        self.ctx._chk(lib.vis_batch_kfdb_match(self._d, C.byref(lp), n, v(d_cand_ptr), cand_stride, max_pts, v(d_matches_ptr), v(d_p1_ptr), v(d_p2_ptr),
                                               v(d_npts_ptr)), "vis_batch_kfdb_match")


class Feeder:
    """pinned-host double-buffered H2D feeder (vis_feeder_*)"""

    def __init__(self, ctx, w, h, batch):
        self.ctx, self.w, self.h, self.batch = ctx, w, h, batch
        self._f = C.c_void_p()
        ctx._chk(lib.vis_feeder_create(ctx._h, w, h, batch, C.byref(self._f)), "vis_feeder_create")

    def host_buffer(self, which):
        p = lib.vis_feeder_host_buffer(self._f, which)
        arr = (C.c_uint8 * (self.batch * self.h * self.w)).from_address(p)
        return np.frombuffer(arr, np.uint8).reshape(self.batch, self.h, self.w)

    def submit(self, which, n):
        d = C.c_void_p()
        self.ctx._chk(lib.vis_feeder_submit(self._f, which, n, C.byref(d)), "vis_feeder_submit")
        return d.value

    def release(self, which):
        self.ctx._chk(lib.vis_feeder_release(self._f, which), "vis_feeder_release")

    def close(self):
        if self._f:
            lib.vis_feeder_destroy(self._f)
            self._f = C.c_void_p()


def synth_canvas(dim=4096, seed=0xE0C00001):
    cv = np.empty((dim, dim), np.uint8)
    rc = lib.vis_synth_canvas(_ptr(cv), dim, C.c_uint64(seed))
    if rc:
        raise VisError(rc, "vis_synth_canvas")
    return cv


def synth_frame(canvas, t, w=752, h=480, seed=0xE0C00001, out=None, parallax=False):
    if out is None:
        out = np.empty((h, w), np.uint8)
    fn = lib.vis_synth_frame_parallax if parallax else lib.vis_synth_frame
    rc = fn(_ptr(canvas), canvas.shape[0], C.c_uint64(seed), int(t), w, h, _ptr(out), out.strides[0])
    if rc:
        raise VisError(rc, "vis_synth_frame")
    return out


class Context:
    """One device context (not thread-safe), like one CameraGPU + MatcherGPU pair."""

    def __init__(self, device=0, params=None):
        self._h = C.c_void_p()
        self._rectifiers = []                                # open Rectify objects: closed before the context
        self._kfdbs = []                                     # open KfDb objects: the same
        rc = lib.vis_create(int(device), C.byref(self._h))
        if rc:
            self._h = None
            raise VisError(rc, "vis_create")
        self.params = default_params()
        if params is not None:
            self.set_params(params)

    def close(self):
        for r in list(getattr(self, "_rectifiers", ())) + list(getattr(self, "_kfdbs", ())):
            r.close()
        if getattr(self, "_h", None):
            lib.vis_destroy(self._h)                         # (synchronises the stream set_stream gave it: released only now)
            self._h = None
        self._stream = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, where):
        if rc:
            raise VisError(rc, where, lib.vis_last_error(self._h).decode())

    def set_params(self, p):
        self._chk(lib.vis_set_params(self._h, C.byref(p)), "vis_set_params")
        self.params = p.copy()

    def set_align_weights(self, aw=None):
        """the weighting every alignment enqueued from now on takes (an AlignWeights; None = the defaults: identity)"""
        self._chk(lib.vis_set_align_weights(self._h, None if aw is None else C.byref(aw)), "vis_set_align_weights")

    def get_align_weights(self):
        aw = AlignWeights()
        self._chk(lib.vis_get_align_weights(self._h, C.byref(aw)), "vis_get_align_weights")
        return aw

    def synth_frames_device(self, d_canvas_ptr, dim, seed, t0, n, w, h, stride, d_out_ptr, parallax=False):
        """frames t0 .. t0+n-1 of the synthetic stream straight into device memory: queued on the context's stream, but the call blocks until
        that stream has drained"""
        self._chk(lib.vis_synth_frames_device(self._h, C.c_void_p(d_canvas_ptr), dim, C.c_uint64(seed), t0, n, w, h, stride,
                                              1 if parallax else 0, C.c_void_p(d_out_ptr)), "vis_synth_frames_device")

    def kfdb(self, entry_cap, kp_cap):
        """vis_kfdb_create: a keyframe database for loop-closure candidates"""
        return KfDb(self, entry_cap, kp_cap)

    def rectify(self, K, dist, Knew, in_size, out_size):
        """vis_rectify_create: the rectification tables of (K, dist) onto K' for in_size -> out_size ((w, h)); close() before the
        context"""
        return Rectify(self, K, dist, Knew, in_size, out_size)

    def set_stream(self, stream):
        """the stream the asynchronous calls enqueue on from now on: a torch.cuda.Stream (anything with a .cuda_stream handle) or a raw
        hipStream_t as an int.  Synchronises: what was queued through the stream set before is complete when this returns.

        The raw handle 0 (or None) selects the context's OWN stream, which is non-blocking: it is NOT ordered with torch's default
        stream, whose handle is 0 as well.  torch's default stream can therefore not be passed -- a stream object whose handle is 0 is
        refused (ValueError) instead of silently selecting the own stream; run the producer on a torch.cuda.Stream() and pass that, or
        synchronise the host.  The stream must outlive the context, or be unset (set_stream(0)) first; the context keeps a reference to
        a stream object it was given."""
        raw = getattr(stream, "cuda_stream", stream)
        if raw is not stream and not raw:
            raise ValueError("the default stream has handle 0, which vis_set_stream reads as 'the context's own stream': pass a torch.cuda.Stream()")
        self._chk(lib.vis_set_stream(self._h, C.c_void_p(int(raw) if raw else None)), "vis_set_stream")
        self._stream = stream if raw else None

    def timings(self):
        t = Timings()
        self._chk(lib.vis_last_timings(self._h, C.byref(t)), "vis_last_timings")
        return t

    def level_geometry(self, w, h):
        L = self.params.nlevels
        ws, hs, q = (np.zeros(L, np.int32) for _ in range(3))
        sc = np.zeros(L, np.float32)
        self._chk(lib.vis_level_geometry(self._h, w, h, _ptr(ws), _ptr(hs), _ptr(sc), _ptr(q)), "vis_level_geometry")
        return ws, hs, sc, q

    def keypoint_capacity(self, w, h):
        """keypoints per frame a plan for w x h frames holds (vis_params.keypoint_capacity): the row length of batch_klt's buffers"""
        q = self.level_geometry(w, h)[3]
        return max(int(sum(int(v) + int(v) // 8 + 32 for v in q)), int(self.params.keypoint_capacity))

    def pyramid_level(self, level, frame=0, batch=False, w=None, h=None):
        """diagnostic: level `level` >= 1 of frame `frame` as the last detection left it -- of the single-frame plan, or of the batch
        plan with batch=True -- as an (h_level, w_level) array without the stride padding.  (w, h) = the frame size of that plan;
        default: the parameters' w_size x h_size"""
        ws, hs, _, _ = self.level_geometry(self.params.w_size if w is None else w, self.params.h_size if h is None else h)
        ok = 0 <= level < len(ws)                                  # (a level the plan does not have: the library refuses it)
        out = np.empty((int(hs[level]), int(ws[level])) if ok else (1, 1), np.uint8)
        self._chk(lib.vis_debug_pyramid_level(self._h, 1 if batch else 0, frame, level, _ptr(out), out.strides[0]), "vis_debug_pyramid_level")
        return out

    # -- Camera::Update --------------------------------------------------------------------------------
    def camera_update(self, img):
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        lw, lh = half_pyramid_dims(w, h)
        levels = [np.empty((lh[l], lw[l]), np.uint8) for l in range(5)]
        arr = (C.c_void_p * 5)(*[l.ctypes.data for l in levels])
        self._chk(lib.vis_camera_update(self._h, _ptr(img), w, h, img.strides[0], arr), "vis_camera_update")
        return levels

    # -- Camera::computeGradient (src/Camera.cpp:167-184) ------------------------------------------------
    def compute_gradient(self, img, scale=3):
        """one host frame -> per level (gx int16, gy int16, gradient u8) of the 5 half-pyramid levels"""
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        lw, lh = half_pyramid_dims(w, h)
        gx = [np.empty((lh[l], lw[l]), np.int16) for l in range(5)]
        gy = [np.empty((lh[l], lw[l]), np.int16) for l in range(5)]
        g = [np.empty((lh[l], lw[l]), np.uint8) for l in range(5)]
        ax = (C.c_void_p * 5)(*[a.ctypes.data for a in gx])
        ay = (C.c_void_p * 5)(*[a.ctypes.data for a in gy])
        ag = (C.c_void_p * 5)(*[a.ctypes.data for a in g])
        self._chk(lib.vis_compute_gradient(self._h, _ptr(img), w, h, img.strides[0], scale, ax, ay, ag), "vis_compute_gradient")
        return gx, gy, g

    def gradient_batch(self, d_frames_ptr, w, h, stride, n, d_gray_ptr, d_gx_ptr, d_gy_ptr, d_g_ptr, scale=3):
        """device pointers in, device buffers out (n * gradient_frame_elems(w, h) elements each); asynchronous"""
        self._chk(lib.vis_gradient_batch(self._h, C.c_void_p(d_frames_ptr), w, h, stride, n, scale, C.c_void_p(d_gray_ptr),
                                         C.c_void_p(d_gx_ptr), C.c_void_p(d_gy_ptr), C.c_void_p(d_g_ptr)), "vis_gradient_batch")

    # -- Camera::ObtainPatchesPointsPreviousFrame / ObtainDebugPointsPreviousFrame (src/Camera.cpp:358-445) --
    def patch_points(self, good, cap=200 * 121):
        good = np.ascontiguousarray(good, KEYPOINT_DTYPE)
        patch = [np.zeros((cap, 4), np.float32) for _ in range(5)]
        debug = [np.zeros((cap, 4), np.float32) for _ in range(5)]
        ap = (C.c_void_p * 5)(*[a.ctypes.data for a in patch])
        ad = (C.c_void_p * 5)(*[a.ctypes.data for a in debug])
        npt = (C.c_int * 5)(); ndb = (C.c_int * 5)()
        self._chk(lib.vis_patch_points(self._h, _ptr(good), len(good), cap, ap, npt, ad, ndb), "vis_patch_points")
        return [patch[l][:npt[l]].copy() for l in range(5)], [debug[l][:ndb[l]].copy() for l in range(5)]

    # -- VISystem::EstimatePoseFeatures (src/VISystem.cpp:1113-1448) ------------------------------------------
    def estimate_pose_features(self, ap, w, h, gray1, gray2, gx1, gy1, cand1, init=None):
        """one pair, host arrays: per-level lists (None for unused levels) -> AlignResult"""
        def lv(arrs, dt):
            keep = [None if a is None else np.ascontiguousarray(a, dt) for a in arrs]
            keep += [None] * (5 - len(keep))
            return keep, (C.c_void_p * 5)(*[None if a is None else a.ctypes.data for a in keep])
        k1, a1 = lv(gray1, np.uint8); k2, a2 = lv(gray2, np.uint8); k3, a3 = lv(gx1, np.int16); k4, a4 = lv(gy1, np.int16)
        k5, a5 = lv(cand1, np.float32)
        n = (C.c_int * 5)(*[0 if c is None else len(c) for c in k5])
        res = AlignResult()
        self._chk(lib.vis_estimate_pose_features(self._h, C.byref(ap), w, h, a1, a2, a3, a4, a5, n,
                                                 None if init is None else C.byref(init), C.byref(res)), "vis_estimate_pose_features")
        return res

    def align_batch(self, ap, d_frames_ptr, w, h, stride, n, d_gray_ptr, d_gx_ptr, d_gy_ptr, d_pts_ptr, d_npts_ptr, max_pts,
                    d_init_ptr, d_out_ptr):
        """device pointers; asynchronous on the context's stream"""
        self._chk(lib.vis_align_batch(self._h, C.byref(ap), C.c_void_p(d_frames_ptr), w, h, stride, n, C.c_void_p(d_gray_ptr),
                                      C.c_void_p(d_gx_ptr), C.c_void_p(d_gy_ptr), C.c_void_p(d_pts_ptr), C.c_void_p(d_npts_ptr), max_pts,
                                      C.c_void_p(d_init_ptr) if d_init_ptr else None, C.c_void_p(d_out_ptr)), "vis_align_batch")

    def batch_align(self, ap, d_frames_ptr, n, d_gray_ptr, d_gx_ptr, d_gy_ptr, d_init_ptr, d_out_ptr):
        """alignment of the pairs of the last batch_run, matched points taken from the plan; asynchronous"""
        nz = lambda q: C.c_void_p(q) if q else None                 # 0 = NULL: gradient pointers all NULL -> the plan's (STAGE_GRADIENT)
        self._chk(lib.vis_batch_align(self._h, C.byref(ap), C.c_void_p(d_frames_ptr), n, nz(d_gray_ptr), nz(d_gx_ptr),
                                      nz(d_gy_ptr), nz(d_init_ptr), C.c_void_p(d_out_ptr)),
                  "vis_batch_align")

    def batch_track_init(self, pose=None):
        """final_poseCam the chain continues from (a Se3f, or None = identity); batch_reset() restarts there.  Synchronises."""
        self._chk(lib.vis_batch_track_init(self._h, C.byref(pose) if pose is not None else None), "vis_batch_track_init")

    def batch_track(self, ap, d_frames_ptr, n, d_init_ptr, d_align_ptr, d_track_ptr):
        """alignment of every frame's keyframe pair of the last batch_run (n AlignResult at d_align_ptr, the pair to the carried
        keyframe included) and VISystem::Track over the frames (n TrackResult at d_track_ptr); device pointers, asynchronous on the
        pose stream like batch_align.  d_init_ptr: n Se3f or 0."""
        self._chk(lib.vis_batch_track(self._h, C.byref(ap), C.c_void_p(d_frames_ptr), n, C.c_void_p(d_init_ptr) if d_init_ptr else None,
                                      C.c_void_p(d_align_ptr), C.c_void_p(d_track_ptr)), "vis_batch_track")

    # -- pyramidal KLT (beyond the reference) -------------------------------------------------------------
    def klt_track(self, w, h, gray1, gx1, gy1, gray2, pts, gx2=None, gy2=None, guess=None, kp=None):
        """one pair, host arrays: per-level lists (None for unused levels; gx2 / gy2 only for forward-backward), pts m x 2 floats
        -> (m records of KLT_POINT_DTYPE, one record of KLT_PAIR_DTYPE)"""
        kp = kp or default_klt_params()

        def lv(arrs, dt):
            if arrs is None:
                return None, None
            keep = [None if a is None else np.ascontiguousarray(a, dt) for a in arrs]
            keep += [None] * (5 - len(keep))
            return keep, (C.c_void_p * 5)(*[None if a is None else a.ctypes.data for a in keep])
        keep = [lv(gray1, np.uint8), lv(gx1, np.int16), lv(gy1, np.int16), lv(gray2, np.uint8), lv(gx2, np.int16), lv(gy2, np.int16)]
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
        guess = None if guess is None else np.ascontiguousarray(guess, np.float32).reshape(len(pts), 2)
        out, pair = np.zeros(len(pts), KLT_POINT_DTYPE), np.zeros(1, KLT_PAIR_DTYPE)
        self._chk(lib.vis_klt_track(self._h, C.byref(kp), w, h, *[k[1] for k in keep], _ptr(pts), _ptr(guess), len(pts), _ptr(out), _ptr(pair)),
                  "vis_klt_track")
        return out, pair[0]

    def klt_batch(self, d_frames_ptr, w, h, stride, n, d_gray_ptr, d_gx_ptr, d_gy_ptr, d_pts_ptr, d_npts_ptr, max_pts, d_out_ptr, d_pair_ptr,
                  d_guess_ptr=0, d_p1_ptr=0, d_p2_ptr=0, d_ntracked_ptr=0, kp=None):
        """device pointers (0 = NULL for the optional ones); asynchronous on the context's stream"""
        kp = kp or default_klt_params()
        nz = lambda q: C.c_void_p(q) if q else None
        self._chk(lib.vis_klt_batch(self._h, C.byref(kp), C.c_void_p(d_frames_ptr), w, h, stride, n, C.c_void_p(d_gray_ptr), C.c_void_p(d_gx_ptr),
                                    C.c_void_p(d_gy_ptr), nz(d_pts_ptr), C.c_void_p(d_npts_ptr), max_pts, nz(d_guess_ptr), nz(d_out_ptr),
                                    C.c_void_p(d_pair_ptr), nz(d_p1_ptr), nz(d_p2_ptr), nz(d_ntracked_ptr)), "vis_klt_batch")

    def batch_klt(self, d_frames_ptr, n, row_cap, d_out_ptr, d_pair_ptr, d_guess_ptr=0, d_p1_ptr=0, d_p2_ptr=0, d_ntracked_ptr=0, kp=None):
        """every keypoint of each pair's previous frame of the last batch_run(DETECT | GRADIENT) tracked into the pair's frame; rows of
        row_cap >= the plan's keypoint capacity; asynchronous on the pose stream like batch_align"""
        kp = kp or default_klt_params()
        nz = lambda q: C.c_void_p(q) if q else None
        self._chk(lib.vis_batch_klt(self._h, C.byref(kp), C.c_void_p(d_frames_ptr), n, nz(d_guess_ptr), row_cap, C.c_void_p(d_out_ptr),
                                    C.c_void_p(d_pair_ptr), nz(d_p1_ptr), nz(d_p2_ptr), nz(d_ntracked_ptr)), "vis_batch_klt")

    # -- CameraGPU::detectAndComputeGPUFeatures ---------------------------------------------------------
    def orb_detect_compute(self, img, slot=0, cap=None):
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        if cap is None:
            cap = 2 * self.params.nfeatures + 1024
        kps = np.zeros(cap, KEYPOINT_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n = C.c_int(0)
        self._chk(lib.vis_orb_detect_compute(self._h, _ptr(img), w, h, img.strides[0], slot, _ptr(kps), _ptr(desc), cap,
                                             C.byref(n)), "vis_orb_detect_compute")
        return kps[:n.value].copy(), desc[:n.value].copy()

    # -- MatcherGPU::computeGPUMatches ---------------------------------------------------------------------
    def bf_knn2_hamming(self, slot_q, slot_t, nq, nt):
        o12 = np.zeros((nq, 2), DMATCH_DTYPE)
        o21 = np.zeros((nt, 2), DMATCH_DTYPE)
        self._chk(lib.vis_bf_knn2_hamming(self._h, slot_q, slot_t, _ptr(o12), _ptr(o21)), "vis_bf_knn2_hamming")
        return o12, o21

    def bf_knn2_hamming_host(self, d1, d2):
        d1 = np.ascontiguousarray(d1, np.uint8).reshape(-1, 32)
        d2 = np.ascontiguousarray(d2, np.uint8).reshape(-1, 32)
        o12 = np.zeros((len(d1), 2), DMATCH_DTYPE)
        o21 = np.zeros((len(d2), 2), DMATCH_DTYPE)
        self._chk(lib.vis_bf_knn2_hamming_host(self._h, _ptr(d1), len(d1), _ptr(d2), len(d2), _ptr(o12), _ptr(o21)),
                  "vis_bf_knn2_hamming_host")
        return o12, o21

    # -- rotation-guided matching: the 2-NN inside the window a rotation predicts (VISystem::WarpFunctionRT + the matcher) --
    def warp_keypoints(self, kps, rot):
        kps = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
        rot = np.ascontiguousarray(rot, np.float32).reshape(9)
        out = np.zeros((len(kps), 2), np.float32)
        self._chk(lib.vis_warp_keypoints(self._h, _ptr(kps), len(kps), _ptr(rot), _ptr(out)), "vis_warp_keypoints")
        return out

    def bf_knn2_hamming_guided(self, slot_q, slot_t, nq, nt, rot, radius):
        rot = np.ascontiguousarray(rot, np.float32).reshape(9)
        o12 = np.zeros((nq, 2), DMATCH_DTYPE)
        o21 = np.zeros((nt, 2), DMATCH_DTYPE)
        self._chk(lib.vis_bf_knn2_hamming_guided(self._h, slot_q, slot_t, _ptr(rot), radius, _ptr(o12), _ptr(o21)), "vis_bf_knn2_hamming_guided")
        return o12, o21

    def bf_knn2_hamming_guided_host(self, d1, k1, d2, k2, rot, radius):
        d1 = np.ascontiguousarray(d1, np.uint8).reshape(-1, 32)
        d2 = np.ascontiguousarray(d2, np.uint8).reshape(-1, 32)
        k1 = np.ascontiguousarray(k1, KEYPOINT_DTYPE)
        k2 = np.ascontiguousarray(k2, KEYPOINT_DTYPE)
        if len(k1) != len(d1) or len(k2) != len(d2):
            raise ValueError("one keypoint per descriptor")
        rot = np.ascontiguousarray(rot, np.float32).reshape(9)
        o12 = np.zeros((len(d1), 2), DMATCH_DTYPE)
        o21 = np.zeros((len(d2), 2), DMATCH_DTYPE)
        self._chk(lib.vis_bf_knn2_hamming_guided_host(self._h, _ptr(d1), _ptr(k1), len(d1), _ptr(d2), _ptr(k2), len(d2), _ptr(rot), radius,
                                                      _ptr(o12), _ptr(o21)), "vis_bf_knn2_hamming_guided_host")
        return o12, o21

    def good_matches_guided(self, slot_prev, slot_cur, rot, radius, sym_cap=65536):
        rot = np.ascontiguousarray(rot, np.float32).reshape(9)
        root2 = 1024
        good = np.zeros(root2, DMATCH_DTYPE)
        sym = np.zeros(sym_cap, DMATCH_DTYPE)
        ng, ns = C.c_int(0), C.c_int(0)
        self._chk(lib.vis_good_matches_guided(self._h, slot_prev, slot_cur, _ptr(rot), radius, _ptr(good), root2, C.byref(ng), _ptr(sym),
                                              sym_cap, C.byref(ns)), "vis_good_matches_guided")
        return good[:ng.value].copy(), sym[:ns.value].copy()

    # -- Matcher::computeBestMatches ----------------------------------------------------------------------
    def good_matches(self, slot_prev, slot_cur, sym_cap=65536):
        root2 = 1024
        good = np.zeros(root2, DMATCH_DTYPE)
        sym = np.zeros(sym_cap, DMATCH_DTYPE)
        ng, ns = C.c_int(0), C.c_int(0)
        self._chk(lib.vis_good_matches(self._h, slot_prev, slot_cur, _ptr(good), root2, C.byref(ng), _ptr(sym), sym_cap,
                                       C.byref(ns)), "vis_good_matches")
        return good[:ng.value].copy(), sym[:ns.value].copy()

    def good_matches_host(self, kps1, kps2, knn12, knn21):
        kps1 = np.ascontiguousarray(kps1, KEYPOINT_DTYPE)
        kps2 = np.ascontiguousarray(kps2, KEYPOINT_DTYPE)
        knn12 = np.ascontiguousarray(knn12, DMATCH_DTYPE)
        knn21 = np.ascontiguousarray(knn21, DMATCH_DTYPE)
        good = np.zeros(1024, DMATCH_DTYPE)
        sym = np.zeros(max(len(kps1), 1), DMATCH_DTYPE)
        ng, ns = C.c_int(0), C.c_int(0)
        self._chk(lib.vis_good_matches_host(self._h, _ptr(kps1), len(kps1), _ptr(kps2), len(kps2), _ptr(knn12), _ptr(knn21),
                                            _ptr(good), 1024, C.byref(ng), _ptr(sym), len(sym), C.byref(ns)),
                  "vis_good_matches_host")
        return good[:ng.value].copy(), sym[:ns.value].copy()

    # -- findEssentialMat / recoverPose --------------------------------------------------------------------
    def essential_ransac(self, p1, p2):
        p1 = np.ascontiguousarray(p1, np.float32).reshape(-1, 2)
        p2 = np.ascontiguousarray(p2, np.float32).reshape(-1, 2)
        E = np.zeros(9, np.float64)
        mask = np.zeros(max(len(p1), 1), np.uint8)
        ni, it = C.c_int(0), C.c_int(0)
        self._chk(lib.vis_essential_ransac(self._h, _ptr(p1), _ptr(p2), len(p1), _ptr(E), _ptr(mask), C.byref(ni), C.byref(it)),
                  "vis_essential_ransac")
        return E.reshape(3, 3), mask[:len(p1)], ni.value, it.value

    def recover_pose(self, E, p1, p2):
        E = np.ascontiguousarray(E, np.float64).reshape(9)
        p1 = np.ascontiguousarray(p1, np.float32).reshape(-1, 2)
        p2 = np.ascontiguousarray(p2, np.float32).reshape(-1, 2)
        R = np.zeros(9, np.float64)
        t = np.zeros(3, np.float64)
        ng = C.c_int(0)
        self._chk(lib.vis_recover_pose(self._h, _ptr(E), _ptr(p1), _ptr(p2), len(p1), _ptr(R), _ptr(t), C.byref(ng)),
                  "vis_recover_pose")
        return R.reshape(3, 3), t, ng.value

    # -- VISystem::Triangulate / Disparity ------------------------------------------------------------------
    def triangulate(self, R, t, p1, p2, mask=None, tp=None):
        """(points MAP_POINT_DTYPE[m], flags uint8[m], TriSummary) of m correspondences under x2 = R x1 + t"""
        R = np.ascontiguousarray(R, np.float64).reshape(9)
        t = np.ascontiguousarray(t, np.float64).reshape(3)
        p1 = np.ascontiguousarray(p1, np.float32).reshape(-1, 2)
        p2 = np.ascontiguousarray(p2, np.float32).reshape(-1, 2)
        m = len(p1)
        if mask is not None:
            mask = np.ascontiguousarray(mask, np.uint8).reshape(-1)
            assert len(mask) == m
        tp = default_tri_params() if tp is None else tp
        pts = np.zeros(max(m, 1), MAP_POINT_DTYPE)
        fl = np.zeros(max(m, 1), np.uint8)
        sm = TriSummary()
        self._chk(lib.vis_triangulate(self._h, C.byref(tp), _ptr(R), _ptr(t), _ptr(p1), _ptr(p2), m, _ptr(mask), _ptr(pts), _ptr(fl),
                                      C.byref(sm)), "vis_triangulate")
        return pts[:m], fl[:m], sm

    def batch_triangulate(self, n, row_cap, d_points_ptr, d_flags_ptr, d_summary_ptr, tp=None):
        """queue the triangulation of every pair of the last batch_run(... | STAGE_POSE) on the pose stream (raw DEVICE pointers: n rows of
        row_cap MapPoint / flag bytes, n TriSummary); the buffers are in use until batch_sync()"""
        tp = default_tri_params() if tp is None else tp
        self._chk(lib.vis_batch_triangulate(self._h, C.byref(tp), n, row_cap, C.c_void_p(d_points_ptr), C.c_void_p(d_flags_ptr),
                                            C.c_void_p(d_summary_ptr)), "vis_batch_triangulate")

    def f2f_ransac(self, pts1, pts2, rot, sample_idx, scale):
        pts1 = np.ascontiguousarray(pts1, KEYPOINT_DTYPE)
        pts2 = np.ascontiguousarray(pts2, KEYPOINT_DTYPE)
        rot = np.ascontiguousarray(rot, np.float32).reshape(9)
        idx = np.ascontiguousarray(sample_idx, np.int32).reshape(-1)
        out = np.zeros(3, np.float32)
        cm = C.c_int(0)
        self._chk(lib.vis_f2f_ransac(self._h, _ptr(pts1), _ptr(pts2), len(pts1), _ptr(rot), _ptr(idx), len(idx) // 2,
                                     C.c_float(scale), _ptr(out), C.byref(cm)), "vis_f2f_ransac")
        return out, cm.value

    # -- VISystem::F2FRansac / FilterKeypoints for the pairs of a batch (raw DEVICE pointers; 0 / None = NULL) ---------------
    def f2f_batch(self, n, d_p1_ptr, d_p2_ptr, d_npts_ptr, max_pts, d_rot_ptr, d_tref_ptr, d_draws_ptr, d_out_ptr):
        """queue F2FRansac of n rows of max_pts (x, y) correspondences on the context's stream: n F2fResult records"""
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_f2f_batch(self._h, n, v(d_p1_ptr), v(d_p2_ptr), v(d_npts_ptr), max_pts, v(d_rot_ptr), v(d_tref_ptr), v(d_draws_ptr),
                                    v(d_out_ptr)), "vis_f2f_batch")

    def batch_f2f(self, n, d_rot_ptr, d_tref_ptr, d_draws_ptr, d_out_ptr):
        """the same on the pairs of the last batch_run(... | STAGE_MATCH), on the pose stream; the buffers are in use until batch_sync()"""
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_batch_f2f(self._h, n, v(d_rot_ptr), v(d_tref_ptr), v(d_draws_ptr), v(d_out_ptr)), "vis_batch_f2f")

    def filter_keypoints_batch(self, n, d_p1_ptr, d_p2_ptr, d_npts_ptr, max_pts, d_rot_ptr, d_t_ptr, threshold, row_cap, d_keep_ptr, d_nkeep_ptr):
        """queue FilterKeypoints of n rows on the context's stream: n rows of row_cap keep bytes and n counts"""
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_filter_keypoints_batch(self._h, n, v(d_p1_ptr), v(d_p2_ptr), v(d_npts_ptr), max_pts, v(d_rot_ptr), v(d_t_ptr),
                                                 float(threshold), row_cap, v(d_keep_ptr), v(d_nkeep_ptr)), "vis_filter_keypoints_batch")

    def batch_filter_keypoints(self, n, d_rot_ptr, d_t_ptr, threshold, row_cap, d_keep_ptr, d_nkeep_ptr):
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_batch_filter_keypoints(self._h, n, v(d_rot_ptr), v(d_t_ptr), float(threshold), row_cap, v(d_keep_ptr), v(d_nkeep_ptr)),
                  "vis_batch_filter_keypoints")

    def filter_keypoints(self, pts1, pts2, rot, t, threshold=500.0):
        """(keep uint8[m], count) of one pair: VISystem::FilterKeypoints with RotationResidual = rot, TranslationResidual = t"""
        pts1 = np.ascontiguousarray(pts1, KEYPOINT_DTYPE)
        pts2 = np.ascontiguousarray(pts2, KEYPOINT_DTYPE)
        assert len(pts1) == len(pts2)
        rot = np.ascontiguousarray(rot, np.float32).reshape(9)
        t = np.ascontiguousarray(t, np.float32).reshape(3)
        keep = np.zeros(max(len(pts1), 1), np.uint8)
        nk = C.c_int(0)
        self._chk(lib.vis_filter_keypoints(self._h, _ptr(pts1), _ptr(pts2), len(pts1), _ptr(rot), _ptr(t), float(threshold), _ptr(keep),
                                           C.byref(nk)), "vis_filter_keypoints")
        return keep[:len(pts1)], nk.value

    # -- homography RANSAC and the H-or-E model choice -----------------------------------------------------------
    def find_homography(self, p1, p2, draws, E=None, hp=None):
        """(record, mask uint8[m]) of one pair: p1 / p2 m x 2 float pixels, draws iters x 4 int32, E 3 x 3 or None; the record is one
        HOMOGRAPHY_RESULT_DTYPE element"""
        hp = default_homography_params() if hp is None else hp
        p1 = np.ascontiguousarray(p1, np.float32).reshape(-1, 2)
        p2 = np.ascontiguousarray(p2, np.float32).reshape(-1, 2)
        assert len(p1) == len(p2)
        draws = np.ascontiguousarray(draws, np.int32).reshape(-1)
        assert len(draws) >= 4 * hp.iters
        E = None if E is None else np.ascontiguousarray(E, np.float64).reshape(9)
        mask = np.zeros(max(len(p1), 1), np.uint8)
        out = np.zeros(1, HOMOGRAPHY_RESULT_DTYPE)
        self._chk(lib.vis_find_homography(self._h, C.byref(hp), _ptr(p1), _ptr(p2), len(p1), _ptr(draws), _ptr(E), _ptr(mask), _ptr(out)),
                  "vis_find_homography")
        return out[0], mask[:len(p1)]

    def homography_batch(self, n, d_p1_ptr, d_p2_ptr, d_npts_ptr, max_pts, d_draws_ptr, d_E_ptr, row_cap, d_mask_ptr, d_out_ptr, hp=None):
        """queue the homography RANSAC of n rows of max_pts (x, y) correspondences on the context's stream (raw DEVICE pointers; 0 / None =
        NULL for d_E and d_mask): n HomographyResult records, n rows of row_cap mask bytes"""
        hp = default_homography_params() if hp is None else hp
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_homography_batch(self._h, C.byref(hp), n, v(d_p1_ptr), v(d_p2_ptr), v(d_npts_ptr), max_pts, v(d_draws_ptr), v(d_E_ptr),
                                           row_cap, v(d_mask_ptr), v(d_out_ptr)), "vis_homography_batch")

    def batch_homography(self, n, d_draws_ptr, row_cap, d_mask_ptr, d_out_ptr, hp=None):
        """the same on the pairs of the last batch_run(... | STAGE_MATCH), on the pose stream, with the pose records' E when that run had
        STAGE_POSE; the buffers are in use until batch_sync()"""
        hp = default_homography_params() if hp is None else hp
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_batch_homography(self._h, C.byref(hp), n, v(d_draws_ptr), row_cap, v(d_mask_ptr), v(d_out_ptr)), "vis_batch_homography")

    # -- the pose of a homography ---------------------------------------------------------------------------------
    def homography_pose(self, hrec, p1, p2, mask=None, rot_hint=None, hq=None):
        """one HPOSE_RESULT_DTYPE element: (R, t / d, n) of the pair's homography record hrec (one HOMOGRAPHY_RESULT_DTYPE element), the
        chosen and the second candidate; p1 / p2 m x 2 float pixels, mask m bytes or None (everyone votes), rot_hint 3 x 3 (current-frame rays
        -> previous frame) or None"""
        hq = default_hpose_params() if hq is None else hq
        p1 = np.ascontiguousarray(p1, np.float32).reshape(-1, 2)
        p2 = np.ascontiguousarray(p2, np.float32).reshape(-1, 2)
        assert len(p1) == len(p2)
        h = np.frombuffer(np.asarray(hrec).tobytes(), HOMOGRAPHY_RESULT_DTYPE).copy()
        assert len(h) == 1
        mask = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(-1)
        assert mask is None or len(mask) >= len(p1)
        rot = None if rot_hint is None else np.ascontiguousarray(rot_hint, np.float32).reshape(9)
        out = np.zeros(1, HPOSE_RESULT_DTYPE)
        self._chk(lib.vis_homography_pose(self._h, C.byref(hq), _ptr(h), _ptr(p1), _ptr(p2), len(p1), _ptr(mask), _ptr(rot), _ptr(out)),
                  "vis_homography_pose")
        return out[0]

    def homography_pose_batch(self, n, d_h_ptr, d_p1_ptr, d_p2_ptr, d_npts_ptr, max_pts, row_cap, d_mask_ptr, d_rot_ptr, d_out_ptr, hq=None):
        """queue the homography pose of n rows of max_pts (x, y) correspondences on the context's stream (raw DEVICE pointers; 0 / None = NULL
        for d_mask and d_rot): n HposeResult records from n HomographyResult records"""
        hq = default_hpose_params() if hq is None else hq
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_homography_pose_batch(self._h, C.byref(hq), n, v(d_h_ptr), v(d_p1_ptr), v(d_p2_ptr), v(d_npts_ptr), max_pts, row_cap,
                                                v(d_mask_ptr), v(d_rot_ptr), v(d_out_ptr)), "vis_homography_pose_batch")

    def batch_homography_pose(self, n, d_h_ptr, row_cap, d_mask_ptr, d_rot_ptr, d_out_ptr, hq=None):
        """the same on the pairs of the last batch_run, from the records and mask rows batch_homography wrote, on the pose stream behind it;
        the buffers are in use until batch_sync()"""
        hq = default_hpose_params() if hq is None else hq
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_batch_homography_pose(self._h, C.byref(hq), n, v(d_h_ptr), row_cap, v(d_mask_ptr), v(d_rot_ptr), v(d_out_ptr)),
                  "vis_batch_homography_pose")

    # -- homography polish: the RANSAC winner refined over its inliers, between the two calls above -----------------
    def homography_polish(self, hrec, p1, p2, mask=None, hp=None):
        """(HPOLISH_RESULT_DTYPE element, mask uint8[m], HOMOGRAPHY_RESULT_DTYPE element): the pair's homography record hrec refined over its
        inliers with the set re-selected, the set the reported H was fitted on, and hrec with the reported H and that set's size --
        homography_pose reads the last two unchanged"""
        hp = default_hpolish_params() if hp is None else hp
        p1 = np.ascontiguousarray(p1, np.float32).reshape(-1, 2)
        p2 = np.ascontiguousarray(p2, np.float32).reshape(-1, 2)
        assert len(p1) == len(p2)
        h = np.frombuffer(np.asarray(hrec).tobytes(), HOMOGRAPHY_RESULT_DTYPE).copy()
        assert len(h) == 1
        mask = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(-1)
        assert mask is None or len(mask) >= len(p1)
        out, ho = np.zeros(1, HPOLISH_RESULT_DTYPE), np.zeros(1, HOMOGRAPHY_RESULT_DTYPE)
        mo = np.zeros(max(len(p1), 1), np.uint8)
        self._chk(lib.vis_homography_polish(self._h, C.byref(hp), _ptr(h), _ptr(p1), _ptr(p2), len(p1), _ptr(mask), _ptr(out), _ptr(mo), _ptr(ho)),
                  "vis_homography_polish")
        return out[0], mo[:len(p1)], ho[0]

    def homography_polish_batch(self, n, d_h_ptr, d_p1_ptr, d_p2_ptr, d_npts_ptr, max_pts, row_cap, d_mask_ptr, d_mask_out_ptr, d_out_ptr,
                                d_h_out_ptr=0, hp=None):
        """queue the polish of n homography records on the context's stream (raw DEVICE pointers; 0 / None = NULL for d_mask and d_h_out):
        homography_pose_batch's buffers, n rows of row_cap output mask bytes, n HPOLISH_RESULT_DTYPE and n HOMOGRAPHY_RESULT_DTYPE records"""
        hp = default_hpolish_params() if hp is None else hp
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_homography_polish_batch(self._h, C.byref(hp), n, v(d_h_ptr), v(d_p1_ptr), v(d_p2_ptr), v(d_npts_ptr), max_pts, row_cap,
                                                  v(d_mask_ptr), v(d_mask_out_ptr), v(d_out_ptr), v(d_h_out_ptr)), "vis_homography_polish_batch")

    def batch_homography_polish(self, n, d_h_ptr, mask_cap, d_mask_ptr, row_cap, d_mask_out_ptr, d_out_ptr, d_h_out_ptr=0, hp=None):
        """the same on the pairs of the last batch_run, from the records and mask rows (mask_cap bytes apart; 0 / None = no mask) batch_homography
        wrote, on the pose stream behind it; batch_homography_pose fed d_h_out and d_mask_out decomposes the polished H.  The buffers are in use
        until batch_sync()"""
        hp = default_hpolish_params() if hp is None else hp
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_batch_homography_polish(self._h, C.byref(hp), n, v(d_h_ptr), mask_cap, v(d_mask_ptr), row_cap, v(d_mask_out_ptr),
                                                  v(d_out_ptr), v(d_h_out_ptr)), "vis_batch_homography_polish")

    # -- PnP: the pose of a frame against map points ---------------------------------------------------------------
    def pnp_ransac(self, X, xy, draws, pp=None):
        """(record, mask uint8[m]) of one problem: X m x 3 double map points, xy m x 2 float pixels, draws iters x 3 int32; the record is one
        PNP_RESULT_DTYPE element"""
        pp = default_pnp_params() if pp is None else pp
        X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        assert len(X) == len(xy)
        draws = np.ascontiguousarray(draws, np.int32).reshape(-1)
        assert len(draws) >= 3 * pp.iters
        mask = np.zeros(max(len(X), 1), np.uint8)
        out = np.zeros(1, PNP_RESULT_DTYPE)
        self._chk(lib.vis_pnp_ransac(self._h, C.byref(pp), _ptr(X), _ptr(xy), len(X), _ptr(draws), _ptr(mask), _ptr(out)), "vis_pnp_ransac")
        return out[0], mask[:len(X)]

    def pnp_batch(self, n, d_X_ptr, x_stride, d_xy_ptr, d_npts_ptr, max_pts, d_draws_ptr, row_cap, d_mask_ptr, d_out_ptr, pp=None):
        """queue the PnP of n rows of max_pts map points (x_stride doubles apart) and pixels on the context's stream (raw DEVICE pointers; 0 /
        None = NULL for d_mask): n PnpResult records, n rows of row_cap mask bytes"""
        pp = default_pnp_params() if pp is None else pp
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_pnp_batch(self._h, C.byref(pp), n, v(d_X_ptr), x_stride, v(d_xy_ptr), v(d_npts_ptr), max_pts, v(d_draws_ptr), row_cap,
                                    v(d_mask_ptr), v(d_out_ptr)), "vis_pnp_batch")

    def batch_pnp(self, n, d_draws_ptr, d_points_ptr, d_flags_ptr, row_cap, d_out_ptr, d_link_ptr, require=16, mask_cap=0, d_mask_ptr=0, pp=None):
        """every frame of the last batch_run(STAGE_ALL) against the map points batch_triangulate wrote for it (d_points / d_flags rows of
        row_cap), on the pose stream behind that call: n PnpResult and n PnpLink records; require = the flag bits a map point must have
        (16 = MP_KEPT); the buffers are in use until batch_sync()"""
        pp = default_pnp_params() if pp is None else pp
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_batch_pnp(self._h, C.byref(pp), n, v(d_draws_ptr), v(d_points_ptr), v(d_flags_ptr), row_cap, require, mask_cap,
                                    v(d_mask_ptr), v(d_out_ptr), v(d_link_ptr)), "vis_batch_pnp")

    # -- feature tracks ---------------------------------------------------------------------------------------------
    def ftrack_link_rows(self, n, d_prev_ptr, d_nkp_ptr, d_links_ptr, d_nlinks_ptr, link_cap, row_cap, d_obs_ptr, d_frame_ptr, seq0=0, d_mask_ptr=0,
                         mask_cap=0, d_carry_in_ptr=0):
        """queue the linking of n frames' match lists (rows of link_cap DMATCH_DTYPE, queryIdx in frame prev[i], trainIdx in frame i) into feature
        tracks on the context's stream (raw DEVICE pointers; 0 / None = NULL for the mask and the carried row): n rows of row_cap FTRACK_OBS_DTYPE
        and n FTRACK_FRAME_DTYPE records"""
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_ftrack_link_rows(self._h, n, v(d_prev_ptr), v(d_nkp_ptr), v(d_links_ptr), v(d_nlinks_ptr), link_cap, v(d_mask_ptr), mask_cap,
                                           v(d_carry_in_ptr), seq0, row_cap, v(d_obs_ptr), v(d_frame_ptr)), "vis_ftrack_link_rows")

    def batch_ftrack(self, n, row_cap, d_obs_ptr, d_frame_ptr, source=FT_SYM, pose_inliers=False, d_mask_ptr=0, mask_cap=0):
        """link the pairs of the last batch_run (with STAGE_MATCH) into feature tracks on the pose stream, continuing the tracks of the launch
        linked before it: n rows of row_cap FTRACK_OBS_DTYPE and n FTRACK_FRAME_DTYPE records, in use until batch_sync()"""
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_batch_ftrack(self._h, source, 1 if pose_inliers else 0, n, v(d_mask_ptr), mask_cap, row_cap, v(d_obs_ptr), v(d_frame_ptr)),
                  "vis_batch_ftrack")

    def ftrack_triangulate_rows(self, n, d_prev_ptr, d_nkp_ptr, d_obs_ptr, row_cap, d_xy_ptr, d_poses_ptr, d_points_ptr, d_flags_ptr, d_summary_ptr,
                                tp=None):
        """queue the N-view triangulation of every track that ends in these n frames on the context's stream (raw DEVICE pointers): d_xy n rows of
        row_cap (u, v) float pixels, d_poses n x 12 doubles (R row-major, t); n rows of row_cap FTRACK_POINT_DTYPE and flag bytes, n
        FTRACK_TRI_SUMMARY_DTYPE records"""
        tp = default_ftrack_tri_params() if tp is None else tp
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_ftrack_triangulate_rows(self._h, C.byref(tp), n, v(d_prev_ptr), v(d_nkp_ptr), v(d_obs_ptr), row_cap, v(d_xy_ptr), v(d_poses_ptr),
                                                  v(d_points_ptr), v(d_flags_ptr), v(d_summary_ptr)), "vis_ftrack_triangulate_rows")

    def batch_ftrack_triangulate(self, n, d_obs_ptr, row_cap, d_poses_ptr, d_points_ptr, d_flags_ptr, d_summary_ptr, tp=None):
        """the same for the keypoints of the last batch_run with the rows batch_ftrack wrote for it, on the pose stream behind that call; the
        buffers are in use until batch_sync()"""
        tp = default_ftrack_tri_params() if tp is None else tp
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_batch_ftrack_triangulate(self._h, C.byref(tp), n, v(d_obs_ptr), row_cap, v(d_poses_ptr), v(d_points_ptr), v(d_flags_ptr),
                                                   v(d_summary_ptr)), "vis_batch_ftrack_triangulate")

    # -- windowed bundle adjustment over the tracks -------------------------------------------------------------------
    def ba_rows(self, n, d_prev_ptr, d_nkp_ptr, d_obs_ptr, row_cap, d_xy_ptr, d_poses_ptr, d_poses_out_ptr, d_windows_ptr, d_points_ptr, d_flags_ptr,
                bp=None):
        """queue the windowed bundle adjustment of these n frames on the context's stream (raw DEVICE pointers): the rows of
        ftrack_triangulate_rows in; n x 12 doubles of refined poses, ba_windows(n, stride) BA_WINDOW_DTYPE records, n rows of row_cap
        BA_POINT_DTYPE and flag bytes out"""
        bp = default_ba_params() if bp is None else bp
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_ba_rows(self._h, C.byref(bp), n, v(d_prev_ptr), v(d_nkp_ptr), v(d_obs_ptr), row_cap, v(d_xy_ptr), v(d_poses_ptr),
                                  v(d_poses_out_ptr), v(d_windows_ptr), v(d_points_ptr), v(d_flags_ptr)), "vis_ba_rows")

    def batch_ba(self, n, d_obs_ptr, row_cap, d_poses_ptr, d_poses_out_ptr, d_windows_ptr, d_points_ptr, d_flags_ptr, bp=None):
        """the same for the keypoints of the last batch_run with the rows batch_ftrack wrote for it, on the pose stream behind that call; the
        buffers are in use until batch_sync()"""
        bp = default_ba_params() if bp is None else bp
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_batch_ba(self._h, C.byref(bp), n, v(d_obs_ptr), row_cap, v(d_poses_ptr), v(d_poses_out_ptr), v(d_windows_ptr),
                                   v(d_points_ptr), v(d_flags_ptr)), "vis_batch_ba")

    # -- a scaled trajectory: scale links between consecutive pairs, and the chain -----------------------------------
    def scale_link_rows(self, n, d_prev_ptr, d_links_ptr, d_nlinks_ptr, link_cap, d_pose_ptr, d_points_ptr, d_flags_ptr, pts_cap, row_cap,
                        d_depth_ptr, d_link_ptr, d_depth_carry_in_ptr=0, sp=None):
        """queue the scale links of n frames of caller rows on the context's stream (raw DEVICE pointers; 0 / None = NULL for the carried depth
        row): n rows of row_cap doubles (the depth rows) and n SCALE_LINK_DTYPE records"""
        sp = default_scale_link_params() if sp is None else sp
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_scale_link_rows(self._h, C.byref(sp), n, v(d_prev_ptr), v(d_links_ptr), v(d_nlinks_ptr), link_cap, v(d_pose_ptr), v(d_points_ptr),
                                          v(d_flags_ptr), pts_cap, v(d_depth_carry_in_ptr), row_cap, v(d_depth_ptr), v(d_link_ptr)), "vis_scale_link_rows")

    def batch_scale_links(self, n, d_points_ptr, d_flags_ptr, row_cap, d_link_ptr, sp=None):
        """the same for the pairs of the last batch_run with the rows batch_triangulate wrote for it, on the pose stream; the plan carries the depth
        row of the last saved frame to the next launch.  n SCALE_LINK_DTYPE records, in use until batch_sync()"""
        sp = default_scale_link_params() if sp is None else sp
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_batch_scale_links(self._h, C.byref(sp), n, v(d_points_ptr), v(d_flags_ptr), row_cap, v(d_link_ptr)), "vis_batch_scale_links")

    def trajectory_rows(self, n, d_prev_ptr, d_pose_ptr, d_link_ptr, d_traj_ptr, d_poses_ptr=0, d_carry_in_ptr=0, seq0=0, same_epoch_only=True):
        """queue the chain of n frames of caller rows on the context's stream: n TRAJ_POSE_DTYPE records and, when d_poses_ptr is given, n x 12
        doubles for ftrack_triangulate_rows / batch_ftrack_triangulate"""
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_trajectory_rows(self._h, n, v(d_prev_ptr), v(d_pose_ptr), v(d_link_ptr), v(d_carry_in_ptr), seq0, 1 if same_epoch_only else 0,
                                          v(d_traj_ptr), v(d_poses_ptr)), "vis_trajectory_rows")

    def batch_trajectory(self, n, d_link_ptr, d_traj_ptr, d_poses_ptr=0, same_epoch_only=True):
        """the same for the frames of the last batch_run with the links batch_scale_links wrote for it, on the pose stream behind that call"""
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_batch_trajectory(self._h, n, v(d_link_ptr), 1 if same_epoch_only else 0, v(d_traj_ptr), v(d_poses_ptr)), "vis_batch_trajectory")

    def batch_trajectory_init(self, rec=None):
        """the record (a TRAJ_POSE_DTYPE element or a TrajPose; None: none) the next run's batch_trajectory continues from; synchronises"""
        if rec is not None and not isinstance(rec, TrajPose):
            rec = TrajPose.from_buffer_copy(np.asarray(rec, TRAJ_POSE_DTYPE).tobytes())
        self._chk(lib.vis_batch_trajectory_init(self._h, C.byref(rec) if rec is not None else None), "vis_batch_trajectory_init")

    # -- IMU preintegration: the rotation and the motion deltas of every pair ------------------------------------------
    def imu_preintegrate(self, samples, t_a, t_b, ip=None):
        """one interval (t_a, t_b] of host samples (IMU_SAMPLE_DTYPE): (an IMU_DELTA_DTYPE record, the 3 x 3 float32 camera-frame rotation); blocks"""
        ip = default_imu_params() if ip is None else ip
        s = np.ascontiguousarray(samples, IMU_SAMPLE_DTYPE)
        d, rot = ImuDelta(), np.zeros(9, np.float32)
        self._chk(lib.vis_imu_preintegrate(self._h, C.byref(ip), C.c_void_p(s.ctypes.data) if len(s) else None, len(s), t_a, t_b, C.byref(d),
                                           C.c_void_p(rot.ctypes.data)), "vis_imu_preintegrate")
        return np.frombuffer(bytes(d), IMU_DELTA_DTYPE)[0], rot.reshape(3, 3)

    def imu_preintegrate_rows(self, n, d_samples_ptr, n_samples, d_tframe_ptr, d_prev_ptr, d_delta_ptr, d_rot_ptr=0, d_carry_in_ptr=0, d_carry_out_ptr=0,
                              ip=None):
        """queue the pair deltas of n frames of caller rows on the context's stream (raw DEVICE pointers; 0 / None = NULL): n IMU_DELTA_DTYPE records,
        n x 9 float32 rotations for batch_f2f / batch_filter_keypoints / batch_run_guided, and the IMU_CARRY_DTYPE record of the next call"""
        ip = default_imu_params() if ip is None else ip
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_imu_preintegrate_rows(self._h, C.byref(ip), n, v(d_samples_ptr), n_samples, v(d_tframe_ptr), v(d_prev_ptr), v(d_carry_in_ptr),
                                                v(d_delta_ptr), v(d_rot_ptr), v(d_carry_out_ptr)), "vis_imu_preintegrate_rows")

    def batch_imu(self, n, d_samples_ptr, n_samples, d_tframe_ptr, d_delta_ptr, d_rot_ptr=0, ip=None):
        """the same for the frames of the last batch_run with batch_get_keyframes' pairing, on the pose stream; the plan carries the open delta and
        the last frame time to the next launch.  The buffers are in use until batch_sync()"""
        ip = default_imu_params() if ip is None else ip
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_batch_imu(self._h, C.byref(ip), n, v(d_samples_ptr), n_samples, v(d_tframe_ptr), v(d_delta_ptr), v(d_rot_ptr)), "vis_batch_imu")

    def batch_imu_init(self, rec=None):
        """the carry (an IMU_CARRY_DTYPE element or an ImuCarry; None: none) the next run's batch_imu continues from; synchronises"""
        if rec is not None and not isinstance(rec, ImuCarry):
            rec = ImuCarry.from_buffer_copy(np.asarray(rec, IMU_CARRY_DTYPE).tobytes())
        self._chk(lib.vis_batch_imu_init(self._h, C.byref(rec) if rec is not None else None), "vis_batch_imu_init")

    # -- the same with the bias Jacobians of v and p, and the first-order bias correction of the records ----------------
    def imu_preintegrate_jac(self, samples, t_a, t_b, ip=None):
        """imu_preintegrate with the Jacobians: (an IMU_DELTA_DTYPE record, an IMU_BIAS_JAC_DTYPE record, the 3 x 3 float32 rotation); blocks"""
        ip = default_imu_params() if ip is None else ip
        s = np.ascontiguousarray(samples, IMU_SAMPLE_DTYPE)
        d, j, rot = ImuDelta(), ImuBiasJac(), np.zeros(9, np.float32)
        self._chk(lib.vis_imu_preintegrate_jac(self._h, C.byref(ip), C.c_void_p(s.ctypes.data) if len(s) else None, len(s), t_a, t_b, C.byref(d), C.byref(j),
                                               C.c_void_p(rot.ctypes.data)), "vis_imu_preintegrate_jac")
        return np.frombuffer(bytes(d), IMU_DELTA_DTYPE)[0], np.frombuffer(bytes(j), IMU_BIAS_JAC_DTYPE)[0], rot.reshape(3, 3)

    def imu_preintegrate_jac_rows(self, n, d_samples_ptr, n_samples, d_tframe_ptr, d_prev_ptr, d_delta_ptr, d_jac_ptr, d_rot_ptr=0, d_carry_in_ptr=0,
                                  d_carry_out_ptr=0, ip=None):
        """imu_preintegrate_rows with n IMU_BIAS_JAC_DTYPE records beside the deltas and IMU_JAC_CARRY_DTYPE carries (raw DEVICE pointers)"""
        ip = default_imu_params() if ip is None else ip
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_imu_preintegrate_jac_rows(self._h, C.byref(ip), n, v(d_samples_ptr), n_samples, v(d_tframe_ptr), v(d_prev_ptr), v(d_carry_in_ptr),
                                                    v(d_delta_ptr), v(d_jac_ptr), v(d_rot_ptr), v(d_carry_out_ptr)), "vis_imu_preintegrate_jac_rows")

    def batch_imu_jac(self, n, d_samples_ptr, n_samples, d_tframe_ptr, d_delta_ptr, d_jac_ptr, d_rot_ptr=0, ip=None):
        """batch_imu with the Jacobians, on the pose stream, with carried records of its own.  The buffers are in use until batch_sync()"""
        ip = default_imu_params() if ip is None else ip
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_batch_imu_jac(self._h, C.byref(ip), n, v(d_samples_ptr), n_samples, v(d_tframe_ptr), v(d_delta_ptr), v(d_jac_ptr), v(d_rot_ptr)),
                  "vis_batch_imu_jac")

    def batch_imu_jac_init(self, rec=None):
        """the carry (an IMU_JAC_CARRY_DTYPE element or an ImuJacCarry; None: none) the next run's batch_imu_jac continues from; synchronises"""
        if rec is not None and not isinstance(rec, ImuJacCarry):
            rec = ImuJacCarry.from_buffer_copy(np.asarray(rec, IMU_JAC_CARRY_DTYPE).tobytes())
        self._chk(lib.vis_batch_imu_jac_init(self._h, C.byref(rec) if rec is not None else None), "vis_batch_imu_jac_init")

    # -- the same with the 9 x 9 covariance of the delta's error --------------------------------------------------------
    def imu_preintegrate_cov(self, samples, t_a, t_b, ip=None, noise=None):
        """imu_preintegrate with the covariance: (an IMU_DELTA_DTYPE record, an IMU_COV_DTYPE record, the 3 x 3 float32 rotation); blocks"""
        ip = default_imu_params() if ip is None else ip
        noise = default_imu_noise() if noise is None else noise
        s = np.ascontiguousarray(samples, IMU_SAMPLE_DTYPE)
        d, c, rot = ImuDelta(), ImuCov(), np.zeros(9, np.float32)
        self._chk(lib.vis_imu_preintegrate_cov(self._h, C.byref(ip), C.byref(noise), C.c_void_p(s.ctypes.data) if len(s) else None, len(s), t_a, t_b, C.byref(d),
                                               C.byref(c), C.c_void_p(rot.ctypes.data)), "vis_imu_preintegrate_cov")
        return np.frombuffer(bytes(d), IMU_DELTA_DTYPE)[0], np.frombuffer(bytes(c), IMU_COV_DTYPE)[0], rot.reshape(3, 3)

    def imu_preintegrate_cov_rows(self, n, d_samples_ptr, n_samples, d_tframe_ptr, d_prev_ptr, d_delta_ptr, d_cov_ptr, d_rot_ptr=0, d_carry_in_ptr=0,
                                  d_carry_out_ptr=0, ip=None, noise=None):
        """imu_preintegrate_rows with n IMU_COV_DTYPE records beside the deltas and IMU_COV_CARRY_DTYPE carries (raw DEVICE pointers)"""
        ip = default_imu_params() if ip is None else ip
        noise = default_imu_noise() if noise is None else noise
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_imu_preintegrate_cov_rows(self._h, C.byref(ip), C.byref(noise), n, v(d_samples_ptr), n_samples, v(d_tframe_ptr), v(d_prev_ptr),
                                                    v(d_carry_in_ptr), v(d_delta_ptr), v(d_cov_ptr), v(d_rot_ptr), v(d_carry_out_ptr)),
                  "vis_imu_preintegrate_cov_rows")

    def batch_imu_cov(self, n, d_samples_ptr, n_samples, d_tframe_ptr, d_delta_ptr, d_cov_ptr, d_rot_ptr=0, ip=None, noise=None):
        """batch_imu with the covariance, on the pose stream, with carried records of its own.  The buffers are in use until batch_sync()"""
        ip = default_imu_params() if ip is None else ip
        noise = default_imu_noise() if noise is None else noise
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_batch_imu_cov(self._h, C.byref(ip), C.byref(noise), n, v(d_samples_ptr), n_samples, v(d_tframe_ptr), v(d_delta_ptr), v(d_cov_ptr),
                                        v(d_rot_ptr)), "vis_batch_imu_cov")

    def batch_imu_cov_init(self, rec=None):
        """the carry (an IMU_COV_CARRY_DTYPE element or an ImuCovCarry; None: none) the next run's batch_imu_cov continues from; synchronises"""
        if rec is not None and not isinstance(rec, ImuCovCarry):
            rec = ImuCovCarry.from_buffer_copy(np.asarray(rec, IMU_COV_CARRY_DTYPE).tobytes())
        self._chk(lib.vis_batch_imu_cov_init(self._h, C.byref(rec) if rec is not None else None), "vis_batch_imu_cov_init")

    def imu_correct_rows(self, n, d_delta_ptr, d_jac_ptr, d_dbg_ptr, d_delta_out_ptr, d_dba_ptr=0, d_rot_out_ptr=0, d_status_ptr=0, ip=None):
        """queue the first-order correction of n records for a bias step on the context's stream (raw DEVICE pointers): d_dbg three doubles (the head
        of a VI_ALIGN_DTYPE record will do), d_dba three doubles or NULL; n corrected IMU_DELTA_DTYPE records, n x 9 float32 rotations, n int32 IMC_*"""
        ip = default_imu_params() if ip is None else ip
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_imu_correct_rows(self._h, C.byref(ip), n, v(d_delta_ptr), v(d_jac_ptr), v(d_dbg_ptr), v(d_dba_ptr), v(d_delta_out_ptr),
                                           v(d_rot_out_ptr), v(d_status_ptr)), "vis_imu_correct_rows")

    def batch_imu_correct(self, n, d_delta_ptr, d_jac_ptr, d_dbg_ptr, d_delta_out_ptr, d_dba_ptr=0, d_rot_out_ptr=0, d_status_ptr=0, ip=None):
        """the same for the frames of the last batch_run on the pose stream, behind batch_vi_align, whose d_result it may read as d_dbg"""
        ip = default_imu_params() if ip is None else ip
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_batch_imu_correct(self._h, C.byref(ip), n, v(d_delta_ptr), v(d_jac_ptr), v(d_dbg_ptr), v(d_dba_ptr), v(d_delta_out_ptr),
                                            v(d_rot_out_ptr), v(d_status_ptr)), "vis_batch_imu_correct")

    # -- visual-inertial alignment: gyro bias, gravity, metric scale, velocities ---------------------------------------
    def vi_align_rows(self, n, d_prev_ptr, d_traj_ptr, d_delta_ptr, d_result_ptr, d_state_ptr=0, d_carry_in_ptr=0, d_carry_out_ptr=0, vp=None):
        """queue the alignment of n frames of caller rows on the context's stream (raw DEVICE pointers; 0 / None = NULL): TRAJ records and
        IMU_DELTA_DTYPE records in, n VI_STATE_DTYPE records, ONE VI_ALIGN_DTYPE record and the VI_CARRY_DTYPE record of the next call out"""
        vp = default_vi_align_params() if vp is None else vp
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_vi_align_rows(self._h, C.byref(vp), n, v(d_prev_ptr), v(d_traj_ptr), v(d_delta_ptr), v(d_carry_in_ptr), v(d_state_ptr),
                                        v(d_result_ptr), v(d_carry_out_ptr)), "vis_vi_align_rows")

    def batch_vi_align(self, n, d_traj_ptr, d_delta_ptr, d_result_ptr, d_state_ptr=0, vp=None):
        """the same for the frames of the last batch_run, behind batch_trajectory and batch_imu of the run, which wrote d_traj and d_delta; the plan
        carries the sums and the tails to the next launch.  The buffers are in use until batch_sync()"""
        vp = default_vi_align_params() if vp is None else vp
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_batch_vi_align(self._h, C.byref(vp), n, v(d_traj_ptr), v(d_delta_ptr), v(d_state_ptr), v(d_result_ptr)), "vis_batch_vi_align")

    # -- the inertial factor of a pair: the delta's residual against the aligned states, whitened by its covariance ---------
    def imu_factor_rows(self, n, d_prev_ptr, d_traj_ptr, d_delta_ptr, d_cov_ptr, d_state_ptr, d_result_ptr, d_factor_ptr, vp=None, fp=None):
        """queue the factors of n frames of caller rows on the context's stream (raw DEVICE pointers): n IMU_FACTOR_DTYPE records from the trajectory
        records, the deltas, their IMU_COV_DTYPE covariances, the VI_STATE_DTYPE states and ONE VI_ALIGN_DTYPE record (or the head of a VI_ALIGN_BA one)"""
        vp = default_vi_align_params() if vp is None else vp
        fp = default_imu_factor_params() if fp is None else fp
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_imu_factor_rows(self._h, C.byref(vp), C.byref(fp), n, v(d_prev_ptr), v(d_traj_ptr), v(d_delta_ptr), v(d_cov_ptr), v(d_state_ptr),
                                          v(d_result_ptr), v(d_factor_ptr)), "vis_imu_factor_rows")

    def batch_imu_factor(self, n, d_traj_ptr, d_delta_ptr, d_cov_ptr, d_state_ptr, d_result_ptr, d_factor_ptr, vp=None, fp=None):
        """the same for the frames of the last batch_run, on the pose stream behind batch_trajectory, batch_imu_cov and batch_vi_align (or _ba) of the
        run, which wrote the inputs.  The buffers are in use until batch_sync()"""
        vp = default_vi_align_params() if vp is None else vp
        fp = default_imu_factor_params() if fp is None else fp
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_batch_imu_factor(self._h, C.byref(vp), C.byref(fp), n, v(d_traj_ptr), v(d_delta_ptr), v(d_cov_ptr), v(d_state_ptr), v(d_result_ptr),
                                           v(d_factor_ptr)), "vis_batch_imu_factor")

    def batch_vi_align_init(self, rec=None):
        """the carry (a VI_CARRY_DTYPE element or a ViCarry; None: none) the next run's batch_vi_align continues from; synchronises"""
        if rec is not None and not isinstance(rec, ViCarry):
            rec = ViCarry.from_buffer_copy(np.asarray(rec, VI_CARRY_DTYPE).tobytes())
        self._chk(lib.vis_batch_vi_align_init(self._h, C.byref(rec) if rec is not None else None), "vis_batch_vi_align_init")

    # -- visual-inertial alignment with the accelerometer bias ---------------------------------------------------------
    def vi_align_ba_rows(self, n, d_prev_ptr, d_traj_ptr, d_delta_ptr, d_jac_ptr, d_result_ptr, d_state_ptr=0, d_carry_in_ptr=0, d_carry_out_ptr=0,
                         vp=None, bp=None):
        """vi_align_rows that also solves for the accelerometer-bias step: IMU_BIAS_JAC_DTYPE records beside the deltas in, n VI_STATE_DTYPE records,
        ONE VI_ALIGN_BA_DTYPE record (its `a` is vi_align_rows' record; d_result + VI_ALIGN_BA_DBA_OFFSET is a d_dba of imu_correct_rows) and the
        VI_BA_CARRY_DTYPE record of the next call out"""
        vp = default_vi_align_params() if vp is None else vp
        bp = default_vi_align_ba_params() if bp is None else bp
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_vi_align_ba_rows(self._h, C.byref(vp), C.byref(bp), n, v(d_prev_ptr), v(d_traj_ptr), v(d_delta_ptr), v(d_jac_ptr),
                                           v(d_carry_in_ptr), v(d_state_ptr), v(d_result_ptr), v(d_carry_out_ptr)), "vis_vi_align_ba_rows")

    def batch_vi_align_ba(self, n, d_traj_ptr, d_delta_ptr, d_jac_ptr, d_result_ptr, d_state_ptr=0, vp=None, bp=None):
        """the same for the frames of the last batch_run, behind batch_trajectory and batch_imu_jac of the run; the plan carries its own sums and
        tails, apart from batch_vi_align's.  batch_imu_correct(..., d_dbg_ptr=d_result_ptr, d_dba_ptr=d_result_ptr + VI_ALIGN_BA_DBA_OFFSET) queued
        behind it applies both estimated steps with no host step.  The buffers are in use until batch_sync()"""
        vp = default_vi_align_params() if vp is None else vp
        bp = default_vi_align_ba_params() if bp is None else bp
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_batch_vi_align_ba(self._h, C.byref(vp), C.byref(bp), n, v(d_traj_ptr), v(d_delta_ptr), v(d_jac_ptr), v(d_state_ptr),
                                            v(d_result_ptr)), "vis_batch_vi_align_ba")

    def batch_vi_align_ba_init(self, rec=None):
        """the carry (a VI_BA_CARRY_DTYPE element or a ViBaCarry; None: none) the next run's batch_vi_align_ba continues from; synchronises"""
        if rec is not None and not isinstance(rec, ViBaCarry):
            rec = ViBaCarry.from_buffer_copy(np.asarray(rec, VI_BA_CARRY_DTYPE).tobytes())
        self._chk(lib.vis_batch_vi_align_ba_init(self._h, C.byref(rec) if rec is not None else None), "vis_batch_vi_align_ba_init")

    # -- the essential-matrix pose on device rows, and its refinement ----------------------------------------------
    def essential_batch(self, n, d_p1_ptr, d_p2_ptr, d_npts_ptr, max_pts, row_cap, d_mask_ptr, d_out_ptr):
        """queue essential RANSAC + recoverPose of n rows of max_pts (x, y) correspondences on the context's stream (raw DEVICE pointers; 0 /
        None = NULL for d_mask): n POSE_RESULT_DTYPE records, n rows of row_cap mask bytes.  The first call, and any call that needs a larger
        workspace, synchronises"""
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_essential_batch(self._h, n, v(d_p1_ptr), v(d_p2_ptr), v(d_npts_ptr), max_pts, row_cap, v(d_mask_ptr), v(d_out_ptr)),
                  "vis_essential_batch")

    def essential_refine(self, R, t, p1, p2, mask=None, ep=None):
        """one EREF_RESULT_DTYPE element: the Gauss-Newton refinement of (R, t) on the Sampson distance over the correspondences p1 / p2 (m x 2
        float pixels) whose mask byte is non-zero (None: all)"""
        ep = default_eref_params() if ep is None else ep
        R = np.ascontiguousarray(R, np.float64).reshape(9)
        t = np.ascontiguousarray(t, np.float64).reshape(3)
        p1 = np.ascontiguousarray(p1, np.float32).reshape(-1, 2)
        p2 = np.ascontiguousarray(p2, np.float32).reshape(-1, 2)
        assert len(p1) == len(p2)
        mask = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(-1)
        assert mask is None or len(mask) >= len(p1)
        out = np.zeros(1, EREF_RESULT_DTYPE)
        self._chk(lib.vis_essential_refine(self._h, C.byref(ep), _ptr(R), _ptr(t), _ptr(p1), _ptr(p2), len(p1), _ptr(mask), _ptr(out)),
                  "vis_essential_refine")
        return out[0]

    def essential_refine_batch(self, n, d_pose_ptr, d_p1_ptr, d_p2_ptr, d_npts_ptr, max_pts, row_cap, d_mask_ptr, d_out_ptr, ep=None):
        """queue the refinement of n pose records on the context's stream (raw DEVICE pointers; 0 / None = NULL for d_mask): exactly the
        buffers essential_batch wrote and read; n EREF_RESULT_DTYPE records"""
        ep = default_eref_params() if ep is None else ep
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_essential_refine_batch(self._h, C.byref(ep), n, v(d_pose_ptr), v(d_p1_ptr), v(d_p2_ptr), v(d_npts_ptr), max_pts, row_cap,
                                                 v(d_mask_ptr), v(d_out_ptr)), "vis_essential_refine_batch")

    def batch_essential_refine(self, n, d_out_ptr, ep=None):
        """the same on the pairs of the last batch_run(STAGE_ALL), from the pose stage's records and inlier mask, on the pose stream behind it;
        d_out is in use until batch_sync().  The refined pose is not written back into the plan"""
        ep = default_eref_params() if ep is None else ep
        self._chk(lib.vis_batch_essential_refine(self._h, C.byref(ep), n, C.c_void_p(d_out_ptr) if d_out_ptr else None), "vis_batch_essential_refine")

    def essential_polish(self, R, t, p1, p2, mask=None, ep=None):
        """(EPOLISH_RESULT_DTYPE element, mask uint8[m], POSE_RESULT_DTYPE element): the refinement of (R, t) with its set re-selected under the
        pose it reached, the set the reported pose was fitted on, and the pose as a record batch_triangulate_from reads"""
        ep = default_epolish_params() if ep is None else ep
        R = np.ascontiguousarray(R, np.float64).reshape(9)
        t = np.ascontiguousarray(t, np.float64).reshape(3)
        p1 = np.ascontiguousarray(p1, np.float32).reshape(-1, 2)
        p2 = np.ascontiguousarray(p2, np.float32).reshape(-1, 2)
        assert len(p1) == len(p2)
        mask = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(-1)
        assert mask is None or len(mask) >= len(p1)
        out, pose = np.zeros(1, EPOLISH_RESULT_DTYPE), np.zeros(1, POSE_RESULT_DTYPE)
        mo = np.zeros(max(len(p1), 1), np.uint8)
        self._chk(lib.vis_essential_polish(self._h, C.byref(ep), _ptr(R), _ptr(t), _ptr(p1), _ptr(p2), len(p1), _ptr(mask), _ptr(out), _ptr(mo),
                                           _ptr(pose)), "vis_essential_polish")
        return out[0], mo[:len(p1)], pose[0]

    def essential_polish_batch(self, n, d_pose_ptr, d_p1_ptr, d_p2_ptr, d_npts_ptr, max_pts, row_cap, d_mask_ptr, d_mask_out_ptr, d_out_ptr,
                               d_pose_out_ptr=0, ep=None):
        """queue the polish of n pose records on the context's stream (raw DEVICE pointers; 0 / None = NULL for d_mask and d_pose_out):
        essential_refine_batch's buffers, n rows of row_cap output mask bytes, n EPOLISH_RESULT_DTYPE and n POSE_RESULT_DTYPE records"""
        ep = default_epolish_params() if ep is None else ep
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_essential_polish_batch(self._h, C.byref(ep), n, v(d_pose_ptr), v(d_p1_ptr), v(d_p2_ptr), v(d_npts_ptr), max_pts, row_cap,
                                                 v(d_mask_ptr), v(d_mask_out_ptr), v(d_out_ptr), v(d_pose_out_ptr)), "vis_essential_polish_batch")

    def batch_essential_polish(self, n, row_cap, d_mask_out_ptr, d_out_ptr, d_pose_out_ptr=0, ep=None):
        """the same on the pairs of the last batch_run(STAGE_ALL), from the pose stage's records and inlier mask (read only), on the pose stream
        behind it; the buffers are in use until batch_sync().  Nothing is written into the plan: batch_triangulate_from reads the outputs"""
        ep = default_epolish_params() if ep is None else ep
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_batch_essential_polish(self._h, C.byref(ep), n, row_cap, v(d_mask_out_ptr), v(d_out_ptr), v(d_pose_out_ptr)),
                  "vis_batch_essential_polish")

    def batch_triangulate_from(self, n, d_pose_ptr, mask_cap, d_mask_ptr, row_cap, d_points_ptr, d_flags_ptr, d_summary_ptr, tp=None):
        """batch_triangulate with the pose records and the mask rows (mask_cap = the plan's correspondences per pair; 0 / None = no mask) taken
        from caller device buffers, e.g. what batch_essential_polish wrote"""
        tp = default_tri_params() if tp is None else tp
        v = lambda a: C.c_void_p(a) if a else None
        self._chk(lib.vis_batch_triangulate_from(self._h, C.byref(tp), n, v(d_pose_ptr), mask_cap, v(d_mask_ptr), row_cap, v(d_points_ptr),
                                                 v(d_flags_ptr), v(d_summary_ptr)), "vis_batch_triangulate_from")

    # -- batched stream path ----------------------------------------------------------------------------------
    def batch_plan(self, w, h, stride, max_frames):
        self._chk(lib.vis_batch_plan(self._h, w, h, stride, max_frames), "vis_batch_plan")

    def batch_reset(self):
        self._chk(lib.vis_batch_reset(self._h), "vis_batch_reset")

    def batch_run(self, dev_ptr, n_frames, stages=STAGE_ALL):
        self._chk(lib.vis_batch_run(self._h, C.c_void_p(dev_ptr), n_frames, stages), "vis_batch_run")

    def batch_run_guided(self, dev_ptr, n_frames, d_rot_ptr, radius, stages=STAGE_ALL):
        """batch_run whose match stage searches inside the window: d_rot_ptr = n_frames x 9 floats in device memory, in use until batch_sync"""
        self._chk(lib.vis_batch_run_guided(self._h, C.c_void_p(dev_ptr), n_frames, stages, C.c_void_p(d_rot_ptr), radius), "vis_batch_run_guided")

    def batch_sync(self):
        self._chk(lib.vis_batch_sync(self._h), "vis_batch_sync")

    def batch_results_async(self, n_cap, h_pose_ptr=None, h_good_ptr=None, h_ngood_ptr=None):
        """queue the D2H copy of the last batch's results (raw host pointers, ideally pinned, holding n_cap frames); the host may
        read them after batch_sync()"""
        self._chk(lib.vis_batch_results_async(self._h, C.c_void_p(h_pose_ptr) if h_pose_ptr else None,
                                              C.c_void_p(h_good_ptr) if h_good_ptr else None,
                                              C.c_void_p(h_ngood_ptr) if h_ngood_ptr else None, n_cap), "vis_batch_results_async")

    def batch_half_pyramid(self):
        """(device pointer, frame_elems) of the half pyramids the last batch_run(..., STAGE_UPDATE) wrote"""
        d, fe = C.c_void_p(0), C.c_size_t(0)
        self._chk(lib.vis_batch_half_pyramid(self._h, C.byref(d), C.byref(fe)), "vis_batch_half_pyramid")
        return d.value, fe.value

    def batch_gradients(self):
        """(gray, gx, gy, g device pointers, frame_elems) of the gradients the last batch_run(..., STAGE_GRADIENT) wrote"""
        p = [C.c_void_p() for _ in range(4)]; fe = C.c_size_t()
        self._chk(lib.vis_batch_gradients(self._h, C.byref(p[0]), C.byref(p[1]), C.byref(p[2]), C.byref(p[3]), C.byref(fe)), "vis_batch_gradients")
        return p[0].value, p[1].value, p[2].value, p[3].value, fe.value

    def batch_results(self, n):
        """synchronous convenience: (pose records, good matches n x root^2, counts) of the last batch"""
        root2 = int(np.floor(np.sqrt(self.params.n_cells))) ** 2
        pose = np.zeros(n, POSE_RESULT_DTYPE); good = np.zeros((n, root2), DMATCH_DTYPE); ng = np.zeros(n, np.int32)
        self.batch_results_async(n, pose.ctypes.data, good.ctypes.data, ng.ctypes.data)
        self.batch_sync()
        return pose, good, ng

    def batch_fast_thresholds(self):
        """(per-level FAST thresholds the next batch starts from, (frame, level) pairs the last batch had to redo)"""
        tau = np.zeros(self.params.nlevels, np.int32)
        nr = C.c_int32(0)
        self._chk(lib.vis_batch_fast_thresholds(self._h, _ptr(tau), C.byref(nr)), "vis_batch_fast_thresholds")
        return tau, nr.value

    def batch_status(self):
        f = C.c_int(0)
        self._chk(lib.vis_batch_status(self._h, C.byref(f)), "vis_batch_status")
        return f.value

    def batch_keypoints(self, frame, cap=None):
        if cap is None:
            cap = 2 * self.params.nfeatures + 1024
        kps = np.zeros(cap, KEYPOINT_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n = C.c_int(0)
        self._chk(lib.vis_batch_get_keypoints(self._h, frame, _ptr(kps), _ptr(desc), cap, C.byref(n)), "vis_batch_get_keypoints")
        return kps[:n.value].copy(), desc[:n.value].copy()

    def batch_knn(self, frame, cap=None):
        if cap is None:
            cap = 2 * self.params.nfeatures + 1024
        o12 = np.zeros((cap, 2), DMATCH_DTYPE)
        o21 = np.zeros((cap, 2), DMATCH_DTYPE)
        n12, n21 = C.c_int(0), C.c_int(0)
        self._chk(lib.vis_batch_get_knn(self._h, frame, _ptr(o12), 2 * cap, C.byref(n12), _ptr(o21), 2 * cap, C.byref(n21)),
                  "vis_batch_get_knn")
        return o12[:n12.value].copy(), o21[:n21.value].copy()

    def batch_matches(self, frame):
        good = np.zeros(1024, DMATCH_DTYPE)
        ng, ns = C.c_int(0), C.c_int(0)
        self._chk(lib.vis_batch_get_matches(self._h, frame, _ptr(good), 1024, C.byref(ng), C.byref(ns)), "vis_batch_get_matches")
        return good[:ng.value].copy(), ns.value

    def debug_counters(self):
        """(kernel launches of the process, host waits of this context's single-frame entry points, asynchronous copies they queued)"""
        out = (C.c_ulonglong * 4)()
        self._chk(lib.vis_debug_counters(self._h, out), "vis_debug_counters")
        return int(out[0]), int(out[1]), int(out[2])

    def undecided_max(self):
        """largest undecided list (vis_pose_result.undecided_max) of any essential_ransac call of this context so far"""
        out = (C.c_ulonglong * 4)()
        self._chk(lib.vis_debug_counters(self._h, out), "vis_debug_counters")
        return int(out[3])

    def batch_inlier_mask(self, frame, cap=16384):
        mask = np.zeros(cap, np.uint8)
        n = C.c_int(0)
        self._chk(lib.vis_batch_get_inlier_mask(self._h, frame, _ptr(mask), cap, C.byref(n)), "vis_batch_get_inlier_mask")
        return mask[:n.value].copy()

    def batch_get_keyframes(self):
        """the pairing of the last batch_run (int32 per frame): the batch index of the frame each frame was matched against, or
        KF_CARRIED / KF_NOT_SAVED / KF_FIRST"""
        n = C.c_int(0)
        self._chk(lib.vis_batch_get_keyframes(self._h, None, 0, C.byref(n)), "vis_batch_get_keyframes")
        prev = np.zeros(n.value, np.int32)
        self._chk(lib.vis_batch_get_keyframes(self._h, _ptr(prev), n.value, C.byref(n)), "vis_batch_get_keyframes")
        return prev

    def batch_pose(self, frame):
        E, R, t = np.zeros(9), np.zeros(9), np.zeros(3)
        ni, ng, it = C.c_int(0), C.c_int(0), C.c_int(0)
        self._chk(lib.vis_batch_get_pose(self._h, frame, _ptr(E), _ptr(R), _ptr(t), C.byref(ni), C.byref(ng), C.byref(it)),
                  "vis_batch_get_pose")
        return dict(E=E.reshape(3, 3), R=R.reshape(3, 3), t=t, n_inliers=ni.value, n_pose_good=ng.value, iters_run=it.value)
