#!/usr/bin/env python3
"""BASELINE configs[0] on a SUPPLIED dataset: the detect -> match -> pose path over the first N frames of an image directory
(EuRoC layout: cam0/data/<timestamp ns>.png, 8-bit greyscale; .pgm / .raw likewise), the way the reference's CPU main walks it
(src/ImageReader.cpp:49-82: sorted listing, imread GRAYSCALE; src/Camera.cpp:127: ORB::create(200)).  No dataset ships with this image and
there is no network: tests/test_ingest.py drives this tool on a synthesised EuRoC-shaped directory; it is here so that a maintainer who HAS
MH_01 can run `python tools/run_directory.py /data/MH_01/mav0/cam0/data --frames 200 --check 20` and read one JSON line.

  frames -> vis_image_read into the feeder's pinned buffers (host decode) -> vis_feeder_submit (H2D on the copy stream)
         -> vis_batch_run(STAGE_FRAME) per batch; results of every frame downloaded.
  --check K: the first K frames also go through the CPU oracle's per-frame pipeline; keypoints, descriptors, good matches and the pose
             record are compared (bit-exact / 1e-7) -- the same checks as tests/test_configs_gpu.py::test_config1...
  --cpu-seconds S: times the oracle on the same frames for about S seconds (the `cpu_baseline` of this dataset).
  --track out.csv: the camera trajectory as the reference's GPU main writes it (src/main_vi_slamGPU.cpp:137-144, its first seven
             columns): one row per frame, positionCam x, y, z, qOrientationCam x, y, z, w -- vis_batch_track after every batch (the
             GPU main's keyframe rule, keyframe_min_points = 1; alignment with the intrinsics of --K fx,fy,cx,cy), from the identity.
  --weights tukey|tukey-signed: with --track, the alignment under the reference's TukeyFunctionWeights (vis_set_align_weights:
             VIS_W_TUKEY as written, VIS_W_TUKEY_SIGNED with signed medians) instead of IdentityWeights.
  --points out.csv: the map points of every frame's pair (vis_batch_triangulate behind every batch, default thresholds): one row per
             correspondence of a pair with a pose -- frame index, timestamp, correspondence index, X, Y, Z (first camera's frame, units
             of the baseline), reproj_px, parallax_px, flags (VIS_MP_*); the JSON line carries the totals.
  --models out.csv: which two-view model explains every frame's pair (vis_batch_homography behind every batch, default parameters, 200
             draws of default_rng(7)): one row per pair -- frame index, timestamp, model (none / homography / essential), n_points,
             n_inliers (H), n_inliers_e, score_h, score_e, best_iter, n_degenerate, H (nine entries, row-major, normalised
             coordinates); the JSON line carries the count of each model.
  --hposes out.csv: the pose of every pair's homography (vis_batch_homography with its mask, then vis_batch_homography_pose without a rotation
             hint, default parameters, the draws of --models): one row per pair -- frame index, timestamp, kind (none / rotation / plane), flags
             (VIS_HPF_*), solution, second, n_points, n_tested, n_parallax, n_good (four), d1, d2, d3, t_norm, then R (nine, row-major), t (in
             units of the plane distance), n of the chosen candidate and R, t, n of the second; the JSON line carries the count of each kind.
  --hpolish: with --hposes, every pair's homography is polished over its inliers before it is decomposed (vis_batch_homography_polish between
             the two calls, default parameters; the pose call reads the polished record and mask): each row of the CSV gains a last column, the
             polish's flags (VIS_HPOL_*), and the JSON line carries the count of each flag.
  --tracks out.csv: the symmetric matches of every pair linked into feature tracks (vis_batch_ftrack behind every batch, the tracks continuing
             across the batches): one row per frame -- frame index, timestamp, the vis_ftrack_frame fields and the histogram of the
             track length at the frame's keypoints (bins 1, 2, 3-4, 5-8, ... 65-); the JSON line carries the totals.
  --trajectory out.csv: the two-view poses of the stream chained under one scale (vis_batch_triangulate, vis_batch_scale_links,
             vis_batch_trajectory, then vis_batch_ftrack and vis_batch_ftrack_triangulate on the trajectory's own d_poses, queued behind every
             batch with no host step between them): one row per frame -- frame index, timestamp, flags, parent, segment_seq, epoch_seq, hops,
             unit_edges, the link's n_shared and flags, its scale, sigma, R (9) and t (3) in the root's frame.
  --pnp out.csv:the pose of every frame against the map points of its keyframe's own pair (vis_batch_triangulate, then vis_batch_pnp with
             VIS_MP_KEPT, default parameters, 200 x 3 draws of default_rng(7)): one row per frame -- frame index, timestamp, q, p, n_linked,
             link flags (VIS_PNPL_*), scale, then n_inliers, n_inliers_refined, best_iter, best_root, flags (VIS_PNP_*), cost0, cost1, R (nine,
             row-major), t (units of the baseline p -> q), R_rel, t_rel; the JSON line carries the counts.
  --refined out.csv: the pose stage's (R, t) of every frame's pair refined over its inlier mask (vis_batch_essential_refine behind every batch,
             default parameters): one row per frame -- frame index, timestamp, flags (VIS_ER_*; 8 = no pair or no pose), n_used, n_points,
             n_inliers0, n_inliers_refined, best_step, steps_run, cost0, cost1, R (nine, row-major), t (unit), E = [t]x R; the JSON line carries
             the counts.
  --polished out.csv: the same pose polished -- its inlier set re-selected at 2 px under the refined pose, up to three times
             (vis_batch_essential_polish behind every batch, default parameters): one row per frame -- frame index, timestamp, flags (VIS_EP_*;
             8 = no pair or no pose), n_points, n_set_first, n_set_last, n_changed, rounds_run, steps_run, best_step, cost_first, cost0, cost1,
             R (nine, row-major), t (unit), E = [t]x R; the JSON line carries the counts.
  --klt out.csv: every keypoint of each pair's previous frame followed into the pair's frame by its image patch (vis_batch_klt behind every
             batch, default parameters with a forward-backward bound of 1 px; adds VIS_STAGE_GRADIENT): one row per point -- frame index,
             timestamp, point index (the keypoint's place in the previous frame's list), x1, y1, x2, y2, flags (VIS_KLT_*), fb, min_eig, sad,
             iters, levels; the JSON line carries the counts.  The pair to a frame of the batch before has no rows (VIS_KLT_NO_PAIR).
  --imu imu0/data.csv --imu-out out.csv: preintegrate the IMU between the frames of every pair on the device (vis_batch_imu behind every batch, the
             plan's own pairing, default parameters; the carry continues across the batches).  The CSV is EuRoC's: timestamp in ns, w (rad/s), a
             (m/s^2), lines that start with # skipped; frame times come from the image file names; both are taken relative to the first frame's
             stamp, in seconds.  One row per frame -- frame index, timestamp, flags (VIS_IMU_*), q, n_steps, dt, R (9), v (3), p (3).
  --ba out.csv: with --trajectory, the windowed bundle adjustment of the chained poses over the feature tracks (vis_batch_ba behind
             vis_batch_trajectory and vis_batch_ftrack, default parameters; the N-view triangulation then reads the adjusted poses): one row per frame
             -- frame, stamp, the flags and the point count of the frame's window, the adjusted R (row-major) and t.  A batch is adjusted on its own:
             observations of earlier batches are not held.
  --loops out.csv [--loop-step K --loop-gap G --loop-entries N]: loop-closure candidates (vis_batch_kfdb_query, _match and _add behind every batch: query
             first, then add, so a frame sees the keyframes of EARLIER batches only; every K-th frame is a query and a keyframe, an entry must be G
             frames older than its query, the database holds the last N keyframes).  The rank-0 candidate's matches go through vis_essential_batch.
             One row per query with a candidate -- frame, stamp, the candidate's frame, score, match count, RANSAC inliers.
  --vi-align out.csv: with --imu and --trajectory, align the chained trajectory with the IMU on the device (vis_batch_vi_align behind
             vis_batch_trajectory and vis_batch_imu of every batch, default parameters; the sums and tails continue across the batches).  One row
             per frame -- frame index, timestamp, flags (VIS_VIS_*), q, res, p (3), v (3), under the batch's own solution; the JSON line carries the
             LAST batch's record: flags (VIS_VIA_*), pairs, triples, dbg, s, g, |g_lin|, rms.
  --imu-jac out.csv: with --imu, integrate with the bias Jacobians of v and p (vis_batch_imu_jac in vis_batch_imu's place: the same deltas).  One row per
             frame -- frame index, timestamp, flags (VIS_IMU_JAC_*), q, Jvg (9), Jva (9), Jpg (9), Jpa (9).
  --imu-cov out.csv [--imu-noise SG,SA]: with --imu, the 9 x 9 covariance of every delta's error (dphi, dv, dp) (vis_batch_imu_cov queued beside the
             integration above, with carried records of its own; SG, SA: the gyro and accelerometer noise densities in rad/s/sqrt(Hz) and
             m/s^2/sqrt(Hz), default EuRoC's 1.6968e-4,2.0e-3).  One row per frame -- frame index, timestamp, flags (VIS_IMU_COV_*), q, the 45 numbers
             of the upper triangle in row order.
  --imu-factor out.csv: with --imu-cov and --vi-align or --vi-align-ba, the inertial factor of every pair (vis_batch_imu_factor queued behind the
             covariance and the alignment of the batch: --vi-align-ba's record and states when both alignments run).  One row per frame -- frame index,
             timestamp, flags (VIS_IMF_*), q, chi2, chi2_rot, r (9); the JSON line counts the solved factors and gives their median chi2.
  --recorrect: with --vi-align and --imu-jac, close the loop on the device: align, correct the batch's deltas for the estimated gyro bias
             (vis_batch_imu_correct reads dbg from the alignment's record), align again on the corrected records.  The states and the JSON record are
             the second alignment's; the JSON line adds the first alignment's dbg, c0_call and c1 and the number of records corrected in the last batch.
  --vi-align-ba out.csv: with --imu, --imu-jac and --trajectory, the alignment that also estimates the accelerometer-bias step (vis_batch_vi_align_ba
             behind vis_batch_trajectory and vis_batch_imu_jac, default parameters, its own carried sums).  One row per frame as for --vi-align, under
             (s_ba, g_ba, dba); the JSON line carries the LAST batch's record: ba_flags (VIS_VIAB_*), flags, pairs, bias triples, dbg, dba, s_ba, g_ba,
             rms_ba.  With --recorrect the correction reads dbg AND dba from the first alignment's record and the second alignment is this call again;
             the JSON line adds dbg_first and dba_first.
  --rectify CALIB.xml: undistort every batch on the device before vis_batch_run (vi::CameraModel, src/CameraModel.cpp:84-105: the
             calibration's in/out_width/height, calibration_values and rectification; K' = getOptimalNewCameraMatrix(alpha = 1)):
             raw frames -> device -> vis_rectify_batch -> the out_width x out_height image, or its window --roi x1,y1,x2,y2
             (VISystem::CalculateROI's rectangle, e.g. 29,54,711,426 for EuRoC) -> vis_batch_run.  K' replaces the intrinsics of
             vis_params and of --track, with its principal point moved into the processed window (cx' - x1, cy' - y1): the frames
             are cropped at (x1, y1), so that is where the rectified camera's centre lies in them; --check runs the oracle on the
             rectified frames the device produced.  (The frames go up through torch, not the feeder: the feeder's frames must
             have the plan's size.)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vi-slam_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (the process's HIP runtime: before the library)
import vislam  # noqa: E402


def read_calibration(path):
    """the fields of a reference-format calibration XML (cv::FileStorage; calibration/calibrationEUROC.xml) that the rectification reads,
    as vi::CameraModel::GetCameraModel reads them (src/CameraModel.cpp:25-68, relative intrinsics scaled by the input size)"""
    import xml.etree.ElementTree as ET
    root = ET.parse(path).getroot()

    def nums(tag):
        el = root.find(tag)
        if el is None:
            raise SystemExit(f"{path}: no <{tag}>")
        data = el.find("data")
        return [float(v) for v in (data if data is not None else el).text.split()]
    c = {t: int(nums(t)[0]) for t in ("in_width", "in_height", "out_width", "out_height")}
    K, dist = nums("calibration_values")[:4], (nums("rectification") + [0.0] * 4)[:4]
    if K[2] < 1 and K[3] < 1:
        K = [K[0] * c["in_width"], K[1] * c["in_height"], K[2] * c["in_width"], K[3] * c["in_height"]]
    c["K"], c["dist"] = tuple(float(v) for v in K), tuple(dist)
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("directory")
    ap.add_argument("--frames", type=int, default=200, help="first N frames of the sorted listing (BASELINE configs[0]: 200)")
    ap.add_argument("--nfeatures", type=int, default=200, help="ORB::create(n): 200 = the reference's CPU main, 1000 = its GPU main")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--check", type=int, default=0, help="compare the first K frames against the CPU oracle")
    ap.add_argument("--cpu-seconds", type=float, default=0.0)
    ap.add_argument("--raw-size", default=None, help="WxH of headerless .raw files")
    ap.add_argument("--track", default=None, metavar="CSV", help="write the per-frame camera pose (positionCam, qOrientationCam) here")
    ap.add_argument("--weights", choices=("identity", "tukey", "tukey-signed"), default="identity",
                    help="--track: the weighting of the alignment's Gauss-Newton step (vis_set_align_weights); identity = the reference's live call")
    ap.add_argument("--points", default=None, metavar="CSV", help="write the triangulated map points of every pair here")
    ap.add_argument("--models", default=None, metavar="CSV", help="write the H-or-E model choice of every pair here")
    ap.add_argument("--hposes", default=None, metavar="CSV", help="write the pose of every pair's homography (chosen and second candidate) here")
    ap.add_argument("--hpolish", action="store_true", help="with --hposes: polish every pair's homography over its inliers before it is decomposed")
    ap.add_argument("--pnp", default=None, metavar="CSV", help="write every frame's pose against its keyframe's map points here")
    ap.add_argument("--refined", default=None, metavar="CSV", help="write every frame's refined two-view pose here")
    ap.add_argument("--polished", default=None, metavar="CSV", help="write every frame's polished two-view pose here")
    ap.add_argument("--klt", default=None, metavar="CSV", help="write the KLT track of every keypoint of every pair here")
    ap.add_argument("--tracks", default=None, metavar="CSV", help="link the symmetric matches into feature tracks; write every frame's summary and length histogram here")
    ap.add_argument("--trajectory", default=None, metavar="CSV", help="chain the two-view poses under the scale links; write one pose per frame here")
    ap.add_argument("--ba", default=None, metavar="CSV", help="with --trajectory: windowed bundle adjustment of the chained poses; one adjusted pose per frame here")
    ap.add_argument("--loops", default=None, metavar="CSV", help="loop-closure candidates of every loop-step-th frame against the keyframe database; one row per query with a candidate")
    ap.add_argument("--loop-step", type=int, default=8)
    ap.add_argument("--loop-gap", type=int, default=30)
    ap.add_argument("--loop-entries", type=int, default=1024)
    ap.add_argument("--imu", default=None, metavar="CSV", help="EuRoC imu0/data.csv: timestamp [ns], w, a")
    ap.add_argument("--imu-out", default=None, metavar="CSV", help="with --imu: write every frame's preintegrated pair delta here")
    ap.add_argument("--imu-jac", default=None, metavar="CSV", help="with --imu: write every frame's bias Jacobians of v and p here")
    ap.add_argument("--imu-cov", default=None, metavar="CSV", help="with --imu: write every frame's 9 x 9 covariance of the delta here")
    ap.add_argument("--imu-noise", default=None, metavar="SG,SA", help="with --imu-cov: the gyro and accelerometer noise densities (default EuRoC's)")
    ap.add_argument("--imu-factor", default=None, metavar="CSV", help="with --imu-cov and --vi-align / --vi-align-ba: write every pair's inertial factor here")
    ap.add_argument("--recorrect", action="store_true", help="with --vi-align and --imu-jac: align, correct the deltas for dbg, align again")
    ap.add_argument("--vi-align-ba", default=None, metavar="CSV", help="with --imu, --imu-jac and --trajectory: align with the accelerometer bias; states here")
    ap.add_argument("--vi-align", default=None, metavar="CSV", help="with --imu and --trajectory: gyro bias, gravity, metric scale; one state per frame here")
    ap.add_argument("--K", default="458.654,457.296,367.215,248.375", help="fx,fy,cx,cy of the alignment (--track); default EuRoC cam0")
    ap.add_argument("--rectify", default=None, metavar="CALIB.xml", help="undistort on the device with this reference-format calibration")
    ap.add_argument("--roi", default=None, metavar="x1,y1,x2,y2", help="with --rectify: the window of the rectified image to process")
    a = ap.parse_args()
    if a.roi and not a.rectify:
        raise SystemExit("--roi needs --rectify")
    if a.hpolish and not a.hposes:
        raise SystemExit("--hpolish needs --hposes")

    names = vislam.image_list(a.directory)[:a.frames]
    if len(names) < 2:
        raise SystemExit(f"{a.directory}: {len(names)} image files (.png / .pgm / .raw)")
    paths = [os.path.join(a.directory, n) for n in names]
    if a.raw_size:
        w, h = (int(x) for x in a.raw_size.lower().split("x"))
    else:
        h, w = vislam.image_read(paths[0]).shape
    stamps = [vislam.image_time(n) for n in names]
    in_w, in_h, window, Kn, Kw = w, h, None, None, None
    if a.rectify:
        cal = read_calibration(a.rectify)
        if (cal["in_width"], cal["in_height"]) != (w, h):
            raise SystemExit(f"{a.rectify}: in_width x in_height {cal['in_width']} x {cal['in_height']}, the images are {w} x {h}")
        if cal["dist"][0] == 0:
            raise SystemExit(f"{a.rectify}: no distortion coefficients (the reference does not rectify then: src/CameraModel.cpp:78-83)")
        Kn = vislam.optimal_new_camera_matrix(cal["K"], cal["dist"], (w, h), (cal["out_width"], cal["out_height"]))
        window = (0, 0, cal["out_width"], cal["out_height"])
        if a.roi:
            x1, y1, x2, y2 = (int(v) for v in a.roi.split(","))
            window = (x1, y1, x2 - x1, y2 - y1)
        w, h = window[2], window[3]
        Kw = (float(Kn[0]), float(Kn[1]), float(Kn[2]) - window[0], float(Kn[3]) - window[1])   # K' in the window's pixel coordinates
    stride = (w + 3) // 4 * 4 if a.rectify else w
    p = vislam.default_params()
    p.nfeatures, p.w_size, p.h_size = a.nfeatures, w, h
    if Kw is not None:
        p.fx, p.cx, p.cy = Kw[0], Kw[2], Kw[3]
    p.fy = p.fx                                              # (the pose stage's one focal length, findEssentialMat(focal = fx))
    stages = vislam.STAGE_FRAME
    if a.track:
        import ctypes as C
        p.keyframe_min_points = 1                            # CameraGPU::addGPUKeyframe's rule
        stages |= vislam.STAGE_GRADIENT
        tap = vislam.default_align_params()
        tap.fx, tap.fy, tap.cx, tap.cy = (float(x) for x in (Kw if Kw is not None else a.K.split(",")))
        d_align = torch.empty(a.batch * C.sizeof(vislam.AlignResult), dtype=torch.uint8, device="cuda")
        d_track = torch.empty(a.batch * C.sizeof(vislam.TrackResult), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        poses = []
    if a.klt:
        stages |= vislam.STAGE_GRADIENT
    ctx = vislam.Context(0, p)
    B = min(a.batch, len(paths))
    ctx.batch_plan(w, h, stride, B)
    if a.klt:
        kltp = vislam.default_klt_params()
        kltp.fb_max_px = 1.0
        kcap = ctx.keypoint_capacity(w, h)
        d_krec = torch.empty(B * kcap * vislam.KLT_POINT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_kpair = torch.empty(B * vislam.KLT_PAIR_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        klt_rows, klt_totals = [], dict(pairs=0, points=0, tracked=0, oob=0, flat=0, fb=0)
    if a.tracks:
        tcap = ctx.keypoint_capacity(w, h)
        d_tobs = torch.empty(B * tcap * vislam.FTRACK_OBS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_tframe = torch.empty(B * vislam.FTRACK_FRAME_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        TRACK_BINS = (1, 2, 3, 5, 9, 17, 33, 65)                # histogram of the track length at a frame: [1], [2], [3, 4], [5, 8], ... [65, inf)
        track_rows, track_totals = [], dict(observations=0, started=0, continued=0, max_len=0, no_carry=0)
    if a.trajectory:                                            # buffers of its own: the chain below is queued whatever else was asked for
        if B > vislam.TJ_MAX_FRAMES:
            raise SystemExit(f"--trajectory chains at most {vislam.TJ_MAX_FRAMES} frames per batch")
        jcap, jk = int(np.floor(np.sqrt(p.n_cells))) ** 2, ctx.keypoint_capacity(w, h)
        z = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        d_jmp, d_jmf, d_jms = z(B * jcap * vislam.MAP_POINT_DTYPE.itemsize), z(B * jcap), z(B * vislam.TRI_SUMMARY_DTYPE.itemsize)
        d_jlink, d_jtraj, d_jposes = z(B * vislam.SCALE_LINK_DTYPE.itemsize), z(B * vislam.TRAJ_POSE_DTYPE.itemsize), z(B * 96)
        d_jobs, d_jframe = z(B * jk * vislam.FTRACK_OBS_DTYPE.itemsize), z(B * vislam.FTRACK_FRAME_DTYPE.itemsize)
        d_jpts, d_jfl, d_jsm = z(B * jk * vislam.FTRACK_POINT_DTYPE.itemsize), z(B * jk), z(B * vislam.FTRACK_TRI_SUMMARY_DTYPE.itemsize)
        traj_rows, traj_totals = [], dict(links_ok=0, roots=0, unit_edges=0, overflow=0, n_view_points=0, n_view_kept=0)
    if a.ba:
        if not a.trajectory:
            raise SystemExit("--ba needs --trajectory")
        bap = vislam.default_ba_params()
        nbw = vislam.ba_windows(B, bap.stride)
        d_bposes, d_bwin = z(B * 96), z(max(nbw, 1) * vislam.BA_WINDOW_DTYPE.itemsize)
        d_bpts, d_bfl = z(B * jk * vislam.BA_POINT_DTYPE.itemsize), z(B * jk)
        ba_rows, ba_totals = [], dict(windows=0, refined=0, few=0, restart=0, no_scale=0, points=0, observations=0, accepted=0, rejected=0, cost0=0.0, cost1=0.0)
    if a.loops:
        if a.loop_step < 1 or a.loop_gap < 0 or not 1 <= a.loop_entries <= 65536:
            raise SystemExit("--loop-step >= 1, --loop-gap >= 0, 1 <= --loop-entries <= 65536")
        lk = ctx.keypoint_capacity(w, h)
        lcap = min(lk, 8192)                                 # (the limit of every RANSAC problem)
        lpp = vislam.default_loop_params()
        lpp.min_gap = a.loop_gap
        ldb = ctx.kfdb(a.loop_entries, lk)
        zl = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        d_lcand, d_lquery = zl(B * lpp.topk * vislam.LOOP_CAND_DTYPE.itemsize), zl(B * vislam.LOOP_QUERY_DTYPE.itemsize)
        d_lp1, d_lp2, d_lnpts, d_lpose = zl(B * lcap * 8), zl(B * lcap * 8), zl(B * 4), zl(B * vislam.POSE_RESULT_DTYPE.itemsize)
        loop_rows, loop_totals = [], dict(queries=0, couples=0, candidates=0, verified=0)
    if a.imu:
        if not a.imu_out:
            raise SystemExit("--imu needs --imu-out")
        if B > vislam.IMU_MAX_FRAMES:
            raise SystemExit(f"--imu integrates at most {vislam.IMU_MAX_FRAMES} frames per batch")
        with open(a.imu) as f:
            lines = [l.split(",") for l in f if l.strip() and not l.startswith("#")]
        imu_s = np.zeros(len(lines), vislam.IMU_SAMPLE_DTYPE)
        for j, l in enumerate(lines):                           # (integer ns less the first frame's stamp: exact in a double, then seconds)
            imu_s[j]["t"], imu_s[j]["w"], imu_s[j]["a"] = (int(l[0]) - stamps[0]) * 1e-9, [float(v) for v in l[1:4]], [float(v) for v in l[4:7]]
        up = lambda arr: torch.from_numpy(np.ascontiguousarray(arr).reshape(-1).view(np.uint8).copy()).cuda()
        d_isamples, d_itf = up(imu_s if len(imu_s) else np.zeros(1, vislam.IMU_SAMPLE_DTYPE)), up(np.asarray([(t - stamps[0]) * 1e-9 for t in stamps], np.float64))
        d_idelta, d_irot = torch.zeros(B * 216, dtype=torch.uint8, device="cuda"), torch.zeros(B * 36, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        imu_rows, imu_totals = [], dict(paired=0, flagged=0)
        if a.imu_jac:
            d_ijac, jac_rows = torch.zeros(B * 296, dtype=torch.uint8, device="cuda"), []
            torch.cuda.synchronize()
        if a.imu_cov:
            d_icov, d_cdelta, cov_rows = torch.zeros(B * 368, dtype=torch.uint8, device="cuda"), torch.zeros(B * 216, dtype=torch.uint8, device="cuda"), []
            noise = vislam.default_imu_noise()
            if a.imu_noise:
                noise.sigma_g, noise.sigma_a = (float(v) for v in a.imu_noise.split(","))
            torch.cuda.synchronize()
    if a.imu_jac and not a.imu:
        raise SystemExit("--imu-jac needs --imu")
    if (a.imu_cov and not a.imu) or (a.imu_noise and not a.imu_cov):
        raise SystemExit("--imu-cov needs --imu, --imu-noise needs --imu-cov")
    if a.imu_factor:
        if not (a.imu_cov and (a.vi_align or a.vi_align_ba)):
            raise SystemExit("--imu-factor needs --imu-cov and --vi-align or --vi-align-ba")
        d_ifac, fac_rows = torch.zeros(B * 96, dtype=torch.uint8, device="cuda"), []
        torch.cuda.synchronize()
    if a.recorrect and not ((a.vi_align or a.vi_align_ba) and a.imu_jac):
        raise SystemExit("--recorrect needs --vi-align and --imu-jac")
    if a.vi_align_ba:
        if not (a.imu and a.imu_jac and a.trajectory):
            raise SystemExit("--vi-align-ba needs --imu-jac and --trajectory")
        d_bstate, d_bres, d_bres1 = (torch.zeros(nbytes, dtype=torch.uint8, device="cuda") for nbytes in (B * 64, 304, 304))
        torch.cuda.synchronize()
        viab_rows, viab_last = [], None
        if a.recorrect:
            d_bdelta2, d_bstatus = (torch.zeros(nbytes, dtype=torch.uint8, device="cuda") for nbytes in (B * 216, B * 4))
            torch.cuda.synchronize()
    if a.vi_align:
        if not (a.imu and a.trajectory):
            raise SystemExit("--vi-align needs --imu and --trajectory")
        d_vstate, d_vres = torch.zeros(B * 64, dtype=torch.uint8, device="cuda"), torch.zeros(160, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        via_rows, via_last = [], None
        if a.recorrect:
            d_idelta2, d_istatus, d_vres1 = (torch.zeros(nbytes, dtype=torch.uint8, device="cuda") for nbytes in (B * 216, B * 4, 160))
            torch.cuda.synchronize()
    if a.weights != "identity":
        aw = vislam.default_align_weights()
        aw.mode = vislam.W_TUKEY if a.weights == "tukey" else vislam.W_TUKEY_SIGNED
        ctx.set_align_weights(aw)
    if a.points or a.pnp:
        row_cap = int(np.floor(np.sqrt(p.n_cells))) ** 2      # the grid-filtered good matches of a pair
        d_mp = torch.empty(B * row_cap * vislam.MAP_POINT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_mf = torch.empty(B * row_cap, dtype=torch.uint8, device="cuda")
        d_ms = torch.empty(B * vislam.TRI_SUMMARY_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        point_rows, tri_totals = [], np.zeros(3, np.int64)
    if a.pnp:
        pp = vislam.default_pnp_params()
        d_pdraws = torch.from_numpy(np.random.default_rng(7).integers(0, 2 ** 31, (pp.iters, 3)).astype(np.int32)).cuda()
        d_prec = torch.empty(B * vislam.PNP_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_plink = torch.empty(B * vislam.PNP_LINK_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        pnp_rows, pnp_totals = [], dict(linked=0, posed=0, refined=0, no_map=0)
    if a.refined:
        erp = vislam.default_eref_params()
        d_eref = torch.empty(B * vislam.EREF_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        eref_rows, eref_totals = [], dict(refined=0, rejected=0, few=0, no_pose=0)
    if a.polished:
        epp = vislam.default_epolish_params()
        pcap = max(int(np.floor(np.sqrt(p.n_cells))) ** 2, 1)  # the grid-filtered good matches of a pair
        d_epol = torch.empty(B * vislam.EPOLISH_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_pmask = torch.empty(B * pcap, dtype=torch.uint8, device="cuda")
        epol_rows, epol_totals = [], dict(polished=0, rejected=0, few=0, no_pose=0, shrank=0)
    if a.models or a.hposes:                                  # one homography RANSAC per batch serves both (the mask does not change the records)
        hp = vislam.default_homography_params()
        d_hdraws = torch.from_numpy(np.random.default_rng(7).integers(0, 2 ** 31, (hp.iters, 4)).astype(np.int32)).cuda()
        d_hrec = torch.empty(B * vislam.HOMOGRAPHY_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        hcap, d_hmask = 0, None
        model_rows, model_totals = [], [0, 0, 0]
    if a.hposes:
        hq = vislam.default_hpose_params()
        hcap = max(int(np.floor(np.sqrt(p.n_cells))) ** 2, 1)  # the grid-filtered good matches of a pair
        d_hmask = torch.empty(B * hcap, dtype=torch.uint8, device="cuda")
        d_hpose = torch.empty(B * vislam.HPOSE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        hpose_rows, hpose_totals = [], [0, 0, 0]
    if a.hpolish:
        hlp = vislam.default_hpolish_params()
        d_hpol = torch.empty(B * vislam.HPOLISH_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_hrec2 = torch.empty(B * vislam.HOMOGRAPHY_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_hmask2 = torch.empty(B * hcap, dtype=torch.uint8, device="cuda")
        hpol_totals = dict(polished=0, rejected=0, few=0, no_model=0, shrank=0)
    torch.cuda.synchronize()
    if a.rectify:
        feed = None
        rect = ctx.rectify(cal["K"], cal["dist"], Kn, (in_w, in_h), (cal["out_width"], cal["out_height"]))
        stage = np.empty((B, in_h, in_w), np.uint8)
        d_rect = [torch.empty(B * h * stride, dtype=torch.uint8, device="cuda") for _ in range(2)]   # double-buffered (--track reads them)
        torch.cuda.synchronize()
    else:
        feed = vislam.Feeder(ctx, w, h, B)
    n = len(paths)
    host = np.empty((n, h, w), np.uint8) if (a.check or a.cpu_seconds > 0) else None
    t_decode = 0.0
    results = []
    t0 = time.perf_counter()
    for bi, first in enumerate(range(0, n, B)):
        k, nb = bi & 1, min(B, n - first)
        buf = feed.host_buffer(k) if feed else stage         # (the feeder's waits until the previous copy out of this buffer is done)
        td = time.perf_counter()
        for i in range(nb):
            buf[i] = vislam.image_read(paths[first + i], in_w, in_h)
            if host is not None and not a.rectify:
                host[first + i] = buf[i]
        t_decode += time.perf_counter() - td
        if feed:
            d = feed.submit(k, nb)
        else:
            d_batch = torch.from_numpy(buf[:nb]).to("cuda")
            torch.cuda.synchronize()                         # (torch's copy and the library's streams are not ordered)
            d = d_rect[k].data_ptr()
            rect.batch(d_batch.data_ptr(), in_w, nb, d, stride, window)
        ctx.batch_run(d, nb, stages)
        if a.track:
            ctx.batch_track(tap, d, nb, 0, d_align.data_ptr(), d_track.data_ptr())
        if a.points or a.pnp:
            ctx.batch_triangulate(nb, row_cap, d_mp.data_ptr(), d_mf.data_ptr(), d_ms.data_ptr())
        if a.pnp:
            ctx.batch_pnp(nb, d_pdraws.data_ptr(), d_mp.data_ptr(), d_mf.data_ptr(), row_cap, d_prec.data_ptr(), d_plink.data_ptr(), vislam.MP_KEPT, 0, 0, pp)
        if a.refined:
            ctx.batch_essential_refine(nb, d_eref.data_ptr(), erp)
        if a.polished:
            ctx.batch_essential_polish(nb, pcap, d_pmask.data_ptr(), d_epol.data_ptr(), 0, epp)
        if a.models or a.hposes:
            ctx.batch_homography(nb, d_hdraws.data_ptr(), hcap, d_hmask.data_ptr() if a.hposes else 0, d_hrec.data_ptr(), hp)
        if a.hpolish:                                        # homography -> polish -> homography_pose, queued on the pose stream: no round trip
            ctx.batch_homography_polish(nb, d_hrec.data_ptr(), hcap, d_hmask.data_ptr(), hcap, d_hmask2.data_ptr(), d_hpol.data_ptr(), d_hrec2.data_ptr(), hlp)
            ctx.batch_homography_pose(nb, d_hrec2.data_ptr(), hcap, d_hmask2.data_ptr(), 0, d_hpose.data_ptr(), hq)
        elif a.hposes:
            ctx.batch_homography_pose(nb, d_hrec.data_ptr(), hcap, d_hmask.data_ptr(), 0, d_hpose.data_ptr(), hq)
        if a.tracks:
            ctx.batch_ftrack(nb, tcap, d_tobs.data_ptr(), d_tframe.data_ptr())
        if a.klt:
            ctx.batch_klt(d, nb, kcap, d_krec.data_ptr(), d_kpair.data_ptr(), kp=kltp)
        if a.imu and a.imu_jac:
            ctx.batch_imu_jac(nb, d_isamples.data_ptr() if len(imu_s) else 0, len(imu_s), d_itf.data_ptr() + 8 * first, d_idelta.data_ptr(), d_ijac.data_ptr(),
                              d_irot.data_ptr())
        elif a.imu:
            ctx.batch_imu(nb, d_isamples.data_ptr() if len(imu_s) else 0, len(imu_s), d_itf.data_ptr() + 8 * first, d_idelta.data_ptr(), d_irot.data_ptr())
        if a.imu and a.imu_cov:                              # (a caller who wants the covariance beside the deltas or the Jacobians queues both)
            ctx.batch_imu_cov(nb, d_isamples.data_ptr() if len(imu_s) else 0, len(imu_s), d_itf.data_ptr() + 8 * first, d_cdelta.data_ptr(), d_icov.data_ptr(),
                              noise=noise)
        if a.trajectory:                                     # run -> triangulate -> scale links -> trajectory -> ftrack -> N-view triangulation: no host step
            ctx.batch_triangulate(nb, jcap, d_jmp.data_ptr(), d_jmf.data_ptr(), d_jms.data_ptr())
            ctx.batch_scale_links(nb, d_jmp.data_ptr(), d_jmf.data_ptr(), jcap, d_jlink.data_ptr())
            ctx.batch_trajectory(nb, d_jlink.data_ptr(), d_jtraj.data_ptr(), d_jposes.data_ptr())
            ctx.batch_ftrack(nb, jk, d_jobs.data_ptr(), d_jframe.data_ptr())
            if a.ba:                                         # ... -> bundle adjustment -> the N-view points under the adjusted poses
                ctx.batch_ba(nb, d_jobs.data_ptr(), jk, d_jposes.data_ptr(), d_bposes.data_ptr(), d_bwin.data_ptr(), d_bpts.data_ptr(), d_bfl.data_ptr(), bap)
            ctx.batch_ftrack_triangulate(nb, d_jobs.data_ptr(), jk, (d_bposes if a.ba else d_jposes).data_ptr(), d_jpts.data_ptr(), d_jfl.data_ptr(),
                                         d_jsm.data_ptr())
        if a.vi_align and a.recorrect:                       # align -> correct by the record's dbg -> align again: queued, no host step
            ctx.batch_vi_align(nb, d_jtraj.data_ptr(), d_idelta.data_ptr(), d_vres1.data_ptr(), d_vstate.data_ptr())
            ctx.batch_imu_correct(nb, d_idelta.data_ptr(), d_ijac.data_ptr(), d_vres1.data_ptr(), d_idelta2.data_ptr(), 0, 0, d_istatus.data_ptr())
            ctx.batch_vi_align(nb, d_jtraj.data_ptr(), d_idelta2.data_ptr(), d_vres.data_ptr(), d_vstate.data_ptr())
        elif a.vi_align:                                     # behind the trajectory and the deltas of the batch, on the same stream
            ctx.batch_vi_align(nb, d_jtraj.data_ptr(), d_idelta.data_ptr(), d_vres.data_ptr(), d_vstate.data_ptr())
        if a.vi_align_ba and a.recorrect:                    # align_ba -> correct by the record's dbg and dba -> align_ba again: queued, no host step
            ctx.batch_vi_align_ba(nb, d_jtraj.data_ptr(), d_idelta.data_ptr(), d_ijac.data_ptr(), d_bres1.data_ptr(), d_bstate.data_ptr())
            ctx.batch_imu_correct(nb, d_idelta.data_ptr(), d_ijac.data_ptr(), d_bres1.data_ptr(), d_bdelta2.data_ptr(),
                                  d_bres1.data_ptr() + vislam.VI_ALIGN_BA_DBA_OFFSET, 0, d_bstatus.data_ptr())
            ctx.batch_vi_align_ba(nb, d_jtraj.data_ptr(), d_bdelta2.data_ptr(), d_ijac.data_ptr(), d_bres.data_ptr(), d_bstate.data_ptr())
        elif a.vi_align_ba:
            ctx.batch_vi_align_ba(nb, d_jtraj.data_ptr(), d_idelta.data_ptr(), d_ijac.data_ptr(), d_bres.data_ptr(), d_bstate.data_ptr())
        if a.imu_factor:                                     # behind the covariance and the alignment of the batch: their buffers, no host step
            d_fres, d_fstate = (d_bres, d_bstate) if a.vi_align_ba else (d_vres, d_vstate)
            ctx.batch_imu_factor(nb, d_jtraj.data_ptr(), d_cdelta.data_ptr(), d_icov.data_ptr(), d_fstate.data_ptr(), d_fres.data_ptr(), d_ifac.data_ptr())
        if a.loops:                                          # query -> the rank-0 candidate's matches -> add: queued on the pose stream, no host step
            ldb.batch_query(nb, 0, d_lcand.data_ptr(), d_lquery.data_ptr(), a.loop_step, lpp)
            ldb.batch_match(nb, d_lcand.data_ptr(), lpp.topk, lcap, 0, d_lp1.data_ptr(), d_lp2.data_ptr(), d_lnpts.data_ptr(), lpp)
            ldb.batch_add(nb, a.loop_step)
        if feed:
            feed.release(k)
        ctx.batch_sync()                                     # (results are fetched per batch below: this harness reports, it does not pipeline)
        if a.loops:                                          # (vis_essential_batch rides the context's stream: behind the synchronisation)
            ctx.essential_batch(nb, d_lp1.data_ptr(), d_lp2.data_ptr(), d_lnpts.data_ptr(), lcap, 0, 0, d_lpose.data_ptr())
            ctx.batch_sync()
            lc = d_lcand.cpu().numpy().view(vislam.LOOP_CAND_DTYPE).reshape(B, lpp.topk)
            lq = d_lquery.cpu().numpy().view(vislam.LOOP_QUERY_DTYPE)
            ln, lpo = d_lnpts.cpu().numpy().view(np.int32), d_lpose.cpu().numpy().view(vislam.POSE_RESULT_DTYPE)
            for i in range(nb):
                if lq[i]["flags"] & vislam.LOOP_SKIPPED:
                    continue
                loop_totals["queries"] += 1
                loop_totals["couples"] += int(lq[i]["n_scored"])
                if lc[i, 0]["slot"] >= 0:
                    loop_totals["candidates"] += 1
                    loop_totals["verified"] += int(lpo[i]["n_inliers"] >= 30)
                    loop_rows.append((first + i, stamps[first + i], int(lc[i, 0]["id"]), int(lc[i, 0]["score"]), int(ln[i]), int(lpo[i]["n_inliers"])))
        if a.rectify and host is not None:                   # --check: the oracle reads the frames the device rectified
            host[first:first + nb] = d_rect[k][:nb * h * stride].cpu().numpy().reshape(nb, h, stride)[:, :, :w]
        if a.track:
            track_bytes = d_track[:nb * C.sizeof(vislam.TrackResult)].cpu().numpy().tobytes()
            poses += [vislam.TrackResult.from_buffer_copy(track_bytes, i * C.sizeof(vislam.TrackResult)).pose for i in range(nb)]
        if a.points:
            mp = d_mp.cpu().numpy().view(vislam.MAP_POINT_DTYPE).reshape(B, row_cap)
            mf, ms = d_mf.cpu().numpy().reshape(B, row_cap), d_ms.cpu().numpy().view(vislam.TRI_SUMMARY_DTYPE)
            for i in range(nb):
                tri_totals += (int(ms[i]["n_points"]), int(ms[i]["n_front"]), int(ms[i]["n_kept"]))
                point_rows += [(first + i, stamps[first + i], j, *mp[i, j]["X"], mp[i, j]["reproj_px"], mp[i, j]["parallax_px"], int(mf[i, j]))
                               for j in range(int(ms[i]["n_points"]))]
        if a.pnp:
            prec, plink = d_prec.cpu().numpy().view(vislam.PNP_RESULT_DTYPE), d_plink.cpu().numpy().view(vislam.PNP_LINK_DTYPE)
            for i in range(nb):
                pnp_totals["linked"] += int(plink[i]["n_linked"] >= 4)
                pnp_totals["posed"] += int(prec[i]["best_iter"] >= 0)
                pnp_totals["refined"] += int(bool(prec[i]["flags"] & vislam.PNP_REFINED))
                pnp_totals["no_map"] += int(bool(plink[i]["flags"] & vislam.PNPL_NO_MAP))
                pnp_rows.append((first + i, stamps[first + i], prec[i].copy(), plink[i].copy()))
        if a.refined:
            erec = d_eref.cpu().numpy().view(vislam.EREF_RESULT_DTYPE)
            for i in range(nb):
                for key, bit in (("refined", vislam.ER_REFINED), ("rejected", vislam.ER_REJECTED), ("few", vislam.ER_FEW), ("no_pose", vislam.ER_NO_POSE)):
                    eref_totals[key] += int(bool(int(erec[i]["flags"]) & bit))
                eref_rows.append((first + i, stamps[first + i], erec[i].copy()))
        if a.polished:
            prec_ = d_epol.cpu().numpy().view(vislam.EPOLISH_RESULT_DTYPE)
            for i in range(nb):
                for key, bit in (("polished", vislam.EP_POLISHED), ("rejected", vislam.EP_REJECTED), ("few", vislam.EP_FEW), ("no_pose", vislam.EP_NO_POSE),
                                 ("shrank", vislam.EP_SHRANK)):
                    epol_totals[key] += int(bool(int(prec_[i]["flags"]) & bit))
                epol_rows.append((first + i, stamps[first + i], prec_[i].copy()))
        if a.models:
            hrec = d_hrec.cpu().numpy().view(vislam.HOMOGRAPHY_RESULT_DTYPE)
            for i in range(nb):
                if int(hrec[i]["n_points"]) > 0:
                    model_totals[int(hrec[i]["model"])] += 1
                    model_rows.append((first + i, stamps[first + i], hrec[i].copy()))
        if a.hposes:
            hpose = d_hpose.cpu().numpy().view(vislam.HPOSE_RESULT_DTYPE)
            hpol = d_hpol.cpu().numpy().view(vislam.HPOLISH_RESULT_DTYPE) if a.hpolish else None
            for i in range(nb):
                if hpol is not None:
                    for key, bit in (("polished", vislam.HPOL_POLISHED), ("rejected", vislam.HPOL_REJECTED), ("few", vislam.HPOL_FEW),
                                     ("no_model", vislam.HPOL_NO_MODEL), ("shrank", vislam.HPOL_SHRANK)):
                        hpol_totals[key] += int(bool(int(hpol[i]["flags"]) & bit))
                if int(hpose[i]["kind"]) != vislam.HP_NONE:
                    hpose_totals[int(hpose[i]["kind"])] += 1
                    hpose_rows.append((first + i, stamps[first + i], hpose[i].copy(), None if hpol is None else int(hpol[i]["flags"])))
        if a.trajectory:
            jl, jt = d_jlink.cpu().numpy().view(vislam.SCALE_LINK_DTYPE), d_jtraj.cpu().numpy().view(vislam.TRAJ_POSE_DTYPE)
            js = d_jsm.cpu().numpy().view(vislam.FTRACK_TRI_SUMMARY_DTYPE)
            for i in range(nb):
                traj_totals["links_ok"] += int(jl[i]["flags"] == vislam.SL_OK and jl[i]["n_shared"] > 0)
                for key, bit in (("roots", vislam.TJ_ROOT), ("unit_edges", vislam.TJ_UNIT_EDGE), ("overflow", vislam.TJ_OVERFLOW)):
                    traj_totals[key] += int(bool(int(jt[i]["flags"]) & bit))
                traj_totals["n_view_points"] += int(js[i]["n_points"])
                traj_totals["n_view_kept"] += int(js[i]["n_kept"])
                traj_rows.append((first + i, stamps[first + i], jt[i].copy(), jl[i].copy()))
        if a.ba:
            bw = d_bwin.cpu().numpy().view(vislam.BA_WINDOW_DTYPE)[:vislam.ba_windows(nb, bap.stride)]
            bpo = d_bposes.cpu().numpy().view(np.float64).reshape(B, 12)
            ba_totals["windows"] += len(bw)
            for key, bit in (("refined", vislam.BA_REFINED), ("few", vislam.BA_FEW), ("restart", vislam.BA_RESTART), ("no_scale", vislam.BA_NO_SCALE)):
                ba_totals[key] += int((bw["flags"] & bit != 0).sum())
            for key, field in (("points", "n_points"), ("observations", "n_obs"), ("accepted", "n_accepted"), ("rejected", "n_rejected")):
                ba_totals[key] += int(bw[field].sum())
            ba_totals["cost0"] += float(bw["cost0"].sum())
            ba_totals["cost1"] += float(bw["cost1"].sum())
            for i in range(nb):
                j = 0 if i == 0 else (i - 1) // bap.stride
                ba_rows.append((first + i, stamps[first + i], int(bw[j]["flags"]), int(bw[j]["n_points"]), bpo[i].copy()))
        if a.imu:
            idl = d_idelta.cpu().numpy().view(vislam.IMU_DELTA_DTYPE)
            for i in range(nb):
                fl = int(idl[i]["flags"])
                imu_totals["paired"] += int(not fl & (vislam.IMU_NO_PAIR | vislam.IMU_NO_CARRY))
                imu_totals["flagged"] += int(bool(fl & ~(vislam.IMU_NO_PAIR | vislam.IMU_NO_CARRY)))
                imu_rows.append((first + i, stamps[first + i], idl[i].copy()))
            if a.imu_jac:
                ijc = d_ijac.cpu().numpy().view(vislam.IMU_BIAS_JAC_DTYPE)
                jac_rows += [(first + i, stamps[first + i], ijc[i].copy()) for i in range(nb)]
            if a.imu_cov:
                icv = d_icov.cpu().numpy().view(vislam.IMU_COV_DTYPE)
                assert d_cdelta.cpu().numpy()[:nb * 216].tobytes() == idl[:nb].tobytes()      # a covariance never changes a delta
                cov_rows += [(first + i, stamps[first + i], icv[i].copy()) for i in range(nb)]
            if a.imu_factor:
                ifc = d_ifac.cpu().numpy().view(vislam.IMU_FACTOR_DTYPE)
                fac_rows += [(first + i, stamps[first + i], ifc[i].copy()) for i in range(nb)]
        if a.vi_align:
            vst, via_last = d_vstate.cpu().numpy().view(vislam.VI_STATE_DTYPE), d_vres.cpu().numpy().view(vislam.VI_ALIGN_DTYPE)[0].copy()
            via_rows += [(first + i, stamps[first + i], vst[i].copy()) for i in range(nb)]
            if a.recorrect:
                via_first = d_vres1.cpu().numpy().view(vislam.VI_ALIGN_DTYPE)[0].copy()
                via_corrected = int((d_istatus.cpu().numpy().view(np.int32)[:nb] == vislam.IMC_OK).sum())
        if a.vi_align_ba:
            bst, viab_last = d_bstate.cpu().numpy().view(vislam.VI_STATE_DTYPE), d_bres.cpu().numpy().view(vislam.VI_ALIGN_BA_DTYPE)[0].copy()
            viab_rows += [(first + i, stamps[first + i], bst[i].copy()) for i in range(nb)]
            if a.recorrect:
                viab_first = d_bres1.cpu().numpy().view(vislam.VI_ALIGN_BA_DTYPE)[0].copy()
                viab_corrected = int((d_bstatus.cpu().numpy().view(np.int32)[:nb] == vislam.IMC_OK).sum())
        if a.tracks:
            tobs = d_tobs.cpu().numpy().view(vislam.FTRACK_OBS_DTYPE).reshape(B, tcap)
            tfr = d_tframe.cpu().numpy().view(vislam.FTRACK_FRAME_DTYPE)
            for i in range(nb):
                f_ = tfr[i]
                lens = tobs[i, :int(f_["n_keypoints"])]["len"]
                hist = np.histogram(lens, bins=TRACK_BINS + (np.iinfo(np.int32).max,))[0]
                track_totals["observations"] += int(f_["n_keypoints"])
                track_totals["started"] += int(f_["n_started"])
                track_totals["continued"] += int(f_["n_continued"])
                track_totals["max_len"] = max(track_totals["max_len"], int(f_["max_len"]))
                track_totals["no_carry"] += int(bool(int(f_["flags"]) & vislam.FT_NO_CARRY))
                track_rows.append((first + i, stamps[first + i], *(int(f_[k]) for k in vislam.FTRACK_FRAME_DTYPE.names), *(int(v) for v in hist)))
        if a.klt:
            krec = d_krec.cpu().numpy().view(vislam.KLT_POINT_DTYPE).reshape(B, kcap)
            kpair, klinks = d_kpair.cpu().numpy().view(vislam.KLT_PAIR_DTYPE), ctx.batch_get_keyframes()
            for i in range(nb):
                if int(kpair[i]["flags"]) & vislam.KLT_NO_PAIR:
                    continue
                src_kp = ctx.batch_keypoints(int(klinks[i]))[0]
                m = int(kpair[i]["n_points"])
                klt_totals["pairs"] += 1
                for key, name in (("points", "n_points"), ("tracked", "n_tracked"), ("oob", "n_oob"), ("flat", "n_flat"), ("fb", "n_fb")):
                    klt_totals[key] += int(kpair[i][name])
                klt_rows += [(first + i, stamps[first + i], j, src_kp["x"][j], src_kp["y"][j], krec[i, j].copy()) for j in range(m)]
        if ctx.batch_status() != 0:
            raise SystemExit("device capacity flag set")
        for i in range(nb):
            kp, ds = ctx.batch_keypoints(i)
            g, nsym = ctx.batch_matches(i)
            results.append((kp, ds, g, nsym, ctx.batch_pose(i)))
    dt = time.perf_counter() - t0
    out = {"directory": a.directory, "frames": n, "width": w, "height": h, "nfeatures": a.nfeatures, "first_timestamp": stamps[0],
           "rectified": None if not a.rectify else {"calibration": a.rectify, "window": list(window), "K_new": [float(v) for v in Kn], "K_window": list(Kw)},
           "median_frame_interval_ns": int(np.median(np.diff(stamps))) if n > 1 else None,
           "frames_per_s_incl_decode_and_downloads": n / dt, "host_decode_s": t_decode, "frames_per_s_host_decode_alone": n / t_decode if t_decode > 0 else None,
           "keypoints_mean": float(np.mean([len(r[0]) for r in results])), "good_matches_mean": float(np.mean([len(r[2]) for r in results[1:]])),
           "inliers_mean": float(np.mean([r[4]["n_inliers"] for r in results[1:]]))}
    if a.check:
        import oracle_bind as orc
        prev, bad = None, []
        for t in range(min(a.check, n)):
            ok, od, r = orc.pipeline_frame(p, host[t], prev)
            kp, ds, g, nsym, pose = results[t]
            same = kp.tobytes() == ok.tobytes() and (ds == od).all() and nsym == r.n_sym and len(g) == r.n_good
            same = same and pose["n_inliers"] == r.n_inliers and pose["iters_run"] == r.iters_run
            if same and r.n_inliers:
                oE = np.array(r.E).reshape(3, 3)
                s = 1.0 if float((pose["E"] * oE).sum()) >= 0 else -1.0
                same = np.abs(pose["E"] - s * oE).max() <= 1e-9 and pose["n_pose_good"] == r.n_pose_good and np.abs(pose["R"] - np.array(r.R).reshape(3, 3)).max() <= 1e-7
            if not same:
                bad.append(t)
            prev = (ok, od)
        out["checked_frames"] = min(a.check, n)
        out["frames_differing_from_the_oracle"] = bad
    if a.cpu_seconds > 0:
        import oracle_bind as orc
        prev, m = None, 0
        tc = time.perf_counter()
        for t in range(n):
            ok, od, _r = orc.pipeline_frame(p, host[t], prev)
            prev = (ok, od)
            m += 1
            if time.perf_counter() - tc > a.cpu_seconds:
                break
        out["cpu_baseline"] = {"value": m / (time.perf_counter() - tc), "unit": "frames/s", "cores": 1, "kind": "port", "sample": f"{m} frames of this directory"}
    if a.track:
        with open(a.track, "w") as f:
            for e in poses:
                f.write(",".join("%.9g" % v for v in (e.tx, e.ty, e.tz, e.qx, e.qy, e.qz, e.qw)) + "\n")
        out["track_csv"] = a.track
    if a.points:
        with open(a.points, "w") as f:
            for r in point_rows:
                f.write("%d,%d,%d,%.17g,%.17g,%.17g,%.9g,%.9g,%d\n" % r)
        out["points_csv"] = a.points
        out["map_points"] = {"triangulated": int(tri_totals[0]), "front": int(tri_totals[1]), "kept": int(tri_totals[2])}
    if a.pnp:
        with open(a.pnp, "w") as f:
            for fi, ts, r, l in pnp_rows:
                ints = [l["q"], l["p"], l["n_linked"], l["flags"]]
                ints2 = [r[k] for k in ("n_inliers", "n_inliers_refined", "best_iter", "best_root", "flags")]
                dbl = [r["cost0"], r["cost1"]] + list(r["R"]) + list(r["t"]) + list(l["R_rel"]) + list(l["t_rel"])
                f.write("%d,%d," % (fi, ts) + ",".join("%d" % v for v in ints) + ",%.17g," % l["scale"] + ",".join("%d" % v for v in ints2) + "," +
                        ",".join("%.17g" % v for v in dbl) + "\n")
        out["pnp_csv"] = a.pnp
        out["pnp"] = pnp_totals
    if a.refined:
        with open(a.refined, "w") as f:
            for fi, ts, r in eref_rows:
                ints = [r[k] for k in ("flags", "n_used", "n_points", "n_inliers0", "n_inliers_refined", "best_step", "steps_run")]
                dbl = [r["cost0"], r["cost1"]] + list(r["R"]) + list(r["t"]) + list(r["E"])
                f.write("%d,%d," % (fi, ts) + ",".join("%d" % v for v in ints) + "," + ",".join("%.17g" % v for v in dbl) + "\n")
        out["refined_csv"] = a.refined
        out["refined"] = eref_totals
    if a.polished:
        with open(a.polished, "w") as f:
            for fi, ts, r in epol_rows:
                ints = [r[k] for k in ("flags", "n_points", "n_set_first", "n_set_last", "n_changed", "rounds_run", "steps_run", "best_step")]
                dbl = [r["cost_first"], r["cost0"], r["cost1"]] + list(r["R"]) + list(r["t"]) + list(r["E"])
                f.write("%d,%d," % (fi, ts) + ",".join("%d" % v for v in ints) + "," + ",".join("%.17g" % v for v in dbl) + "\n")
        out["polished_csv"] = a.polished
        out["polished"] = epol_totals
    if a.models:
        with open(a.models, "w") as f:
            for fi, ts, r in model_rows:
                f.write("%d,%d,%s,%d,%d,%d,%.17g,%.17g,%d,%d," % (fi, ts, vislam.MODEL_NAMES[int(r["model"])], r["n_points"], r["n_inliers"], r["n_inliers_e"],
                                                                   r["score_h"], r["score_e"], r["best_iter"], r["n_degenerate"])
                        + ",".join("%.17g" % v for v in r["H"]) + "\n")
        out["models_csv"] = a.models
        out["models"] = dict(zip(vislam.MODEL_NAMES, model_totals))
    if a.trajectory:
        with open(a.trajectory, "w") as f:                      # frame, stamp, the vis_traj_pose integers, the link's n_shared and flags, scale, sigma, R, t
            for fi, ts, r, l in traj_rows:
                ints = [r[k] for k in ("flags", "parent", "segment_seq", "epoch_seq", "hops", "unit_edges")] + [l["n_shared"], l["flags"]]
                dbl = [l["scale"], r["sigma"]] + list(r["R"]) + list(r["t"])
                f.write("%d,%d," % (fi, ts) + ",".join("%d" % v for v in ints) + "," + ",".join("%.17g" % v for v in dbl) + "\n")
        out["trajectory_csv"] = a.trajectory
        out["trajectory"] = traj_totals
    if a.ba:
        with open(a.ba, "w") as f:                              # frame, stamp, its window's flags and points, the adjusted R, t
            for fi, ts, wf, wn, pose in ba_rows:
                f.write("%d,%d,%d,%d," % (fi, ts, wf, wn) + ",".join("%.17g" % v for v in pose) + "\n")
        out["ba_csv"] = a.ba
        out["ba"] = ba_totals
    if a.loops:
        with open(a.loops, "w") as f:                           # frame, stamp, the candidate's frame, score, matches, RANSAC inliers
            for row in loop_rows:
                f.write("%d,%d,%d,%d,%d,%d\n" % row)
        out["loops_csv"] = a.loops
        out["loops"] = loop_totals
    if a.imu:
        with open(a.imu_out, "w") as f:                         # frame, stamp, flags, q, n_steps, dt, R, v, p
            for fi, ts, r in imu_rows:
                dbl = [r["dt"]] + list(r["R"]) + list(r["v"]) + list(r["p"])
                f.write("%d,%d,%d,%d,%d," % (fi, ts, r["flags"], r["q"], r["n_steps"]) + ",".join("%.17g" % v for v in dbl) + "\n")
        out["imu_csv"] = a.imu_out
        out["imu"] = dict(imu_totals, samples=len(imu_s))
        if a.imu_jac:
            with open(a.imu_jac, "w") as f:                     # frame, stamp, flags, q, Jvg, Jva, Jpg, Jpa
                for fi, ts, r in jac_rows:
                    dbl = list(r["Jvg"]) + list(r["Jva"]) + list(r["Jpg"]) + list(r["Jpa"])
                    f.write("%d,%d,%d,%d," % (fi, ts, r["flags"], r["q"]) + ",".join("%.17g" % v for v in dbl) + "\n")
            out["imu_jac_csv"] = a.imu_jac
        if a.imu_cov:
            with open(a.imu_cov, "w") as f:                     # frame, stamp, flags, q, the 45 of the upper triangle
                for fi, ts, r in cov_rows:
                    f.write("%d,%d,%d,%d," % (fi, ts, r["flags"], r["q"]) + ",".join("%.17g" % v for v in r["S"]) + "\n")
            out["imu_cov_csv"] = a.imu_cov
            out["imu_noise"] = [noise.sigma_g, noise.sigma_a]
        if a.imu_factor:
            with open(a.imu_factor, "w") as f:                  # frame, stamp, flags, q, chi2, chi2_rot, r
                for fi, ts, r in fac_rows:
                    f.write("%d,%d,%d,%d," % (fi, ts, r["flags"], r["q"]) + ",".join("%.17g" % v for v in [r["chi2"], r["chi2_rot"]] + list(r["r"])) + "\n")
            solved = [float(r["chi2"]) for _, _, r in fac_rows if int(r["flags"]) == 0]
            out["imu_factor_csv"] = a.imu_factor
            out["imu_factor"] = dict(solved=len(solved), median_chi2=float(np.median(solved)) if solved else None)
    if a.vi_align:
        with open(a.vi_align, "w") as f:                        # frame, stamp, flags, q, res, p, v
            for fi, ts, r in via_rows:
                f.write("%d,%d,%d,%d," % (fi, ts, r["flags"], r["q"]) + ",".join("%.17g" % v for v in [r["res"]] + list(r["p"]) + list(r["v"])) + "\n")
        out["vi_align_csv"] = a.vi_align
        if via_last is not None:
            out["vi_align"] = dict(flags=int(via_last["flags"]), pairs=int(via_last["n_pairs"]), triples=int(via_last["n_triples"]),
                                   dbg=[float(v) for v in via_last["dbg"]], s=float(via_last["s"]), g=[float(v) for v in via_last["g"]],
                                   g_lin_norm=float(via_last["g_lin_norm"]), rms=float(via_last["rms"]))
            if a.recorrect:
                out["recorrect"] = dict(dbg_first=[float(v) for v in via_first["dbg"]], c0_call_first=float(via_first["c0_call"]),
                                        c1_first=float(via_first["c1"]), c0_call=float(via_last["c0_call"]), corrected_in_the_last_batch=via_corrected)
    if a.vi_align_ba:
        with open(a.vi_align_ba, "w") as f:                     # frame, stamp, flags, q, res, p, v
            for fi, ts, r in viab_rows:
                f.write("%d,%d,%d,%d," % (fi, ts, r["flags"], r["q"]) + ",".join("%.17g" % v for v in [r["res"]] + list(r["p"]) + list(r["v"])) + "\n")
        out["vi_align_ba_csv"] = a.vi_align_ba
        if viab_last is not None:
            r = viab_last
            out["vi_align_ba"] = dict(ba_flags=int(r["ba_flags"]), flags=int(r["a"]["flags"]), pairs=int(r["a"]["n_pairs"]), bias_triples=int(r["n_ba_triples"]),
                                      dbg=[float(v) for v in r["a"]["dbg"]], dba=[float(v) for v in r["dba"]], s_ba=float(r["s_ba"]),
                                      g_ba=[float(v) for v in r["g_ba"]], rms_ba=float(r["rms_ba"]))
            if a.recorrect:
                rc = dict(dbg_first=[float(v) for v in viab_first["a"]["dbg"]], dba_first=[float(v) for v in viab_first["dba"]],
                          corrected_in_the_last_batch=viab_corrected)
                out["recorrect"] = dict(out.get("recorrect", {}), **rc)
    if a.tracks:
        with open(a.tracks, "w") as f:                         # frame, stamp, the vis_ftrack_frame fields, the histogram of len over TRACK_BINS
            for r in track_rows:
                f.write(",".join("%d" % v for v in r) + "\n")
        out["tracks_csv"] = a.tracks
        out["tracks"] = dict(track_totals, mean_len=track_totals["observations"] / max(track_totals["started"], 1), histogram_bins=list(TRACK_BINS))
    if a.klt:
        with open(a.klt, "w") as f:
            for fi, ts, j, x1, y1, r in klt_rows:
                f.write("%d,%d,%d,%.9g,%.9g,%.9g,%.9g,%d,%.9g,%.9g,%d,%d,%d\n" % (fi, ts, j, x1, y1, r["x"], r["y"], r["flags"], r["fb"], r["min_eig"],
                                                                                   r["sad"], r["iters"], r["levels"]))
        out["klt_csv"] = a.klt
        out["klt"] = klt_totals
    if a.hposes:
        with open(a.hposes, "w") as f:
            for fi, ts, r, pflags in hpose_rows:
                ints = [r[k] for k in ("flags", "solution", "second", "n_points", "n_tested", "n_parallax")] + list(r["n_good"])
                dbl = list(r["sv"]) + [r["t_norm"]] + [v for k in ("R", "t", "n", "R2", "t2", "n2") for v in r[k]]
                f.write("%d,%d,%s," % (fi, ts, vislam.HP_KIND_NAMES[int(r["kind"])]) + ",".join("%d" % v for v in ints) + "," +
                        ",".join("%.17g" % v for v in dbl) + ("" if pflags is None else ",%d" % pflags) + "\n")
        out["hposes_csv"] = a.hposes
        out["hposes"] = dict(zip(vislam.HP_KIND_NAMES, hpose_totals))
        if a.hpolish:
            out["hpolish"] = hpol_totals
    if feed:
        feed.close()
    else:
        rect.close()
    ctx.close()
    print(json.dumps(out, allow_nan=False))
    return 1 if out.get("frames_differing_from_the_oracle") else 0


if __name__ == "__main__":
    sys.exit(main())
