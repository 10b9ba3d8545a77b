"""The oracle's side of the batched camera tracking, shared by the test modules that check vis_batch_track (tests/test_batch_track_gpu.py,
tests/test_stride_range_gpu.py, tests/test_align_hostile_gpu.py).  Not a test module.

  decode     the device's alignment and track records as ctypes structures, and their bytes
  residual   the pose VISystem::Track composes: SE3(matrix(pose).R, pose.t)
  Oracle     EstimatePoseFeatures (previous -> current) on the matched keypoints of the previous frame, cached"""
import ctypes as C

W, H = 752, 480


def decode(vislam, a, t, n):
    ra, rt = a.cpu().numpy().tobytes(), t.cpu().numpy().tobytes()
    sa, st = C.sizeof(vislam.AlignResult), C.sizeof(vislam.TrackResult)
    return ([vislam.AlignResult.from_buffer_copy(ra, i * sa) for i in range(n)], [vislam.TrackResult.from_buffer_copy(rt, i * st) for i in range(n)],
            ra, rt)


def residual(orc, pose):
    M = orc.se3_matrix(pose)
    return orc.se3_from_rt(M[:3, :3], M[:3, 3])


class Oracle:
    """EstimatePoseFeatures (prev -> cur) on the matched keypoints of prev, cached by pair and points; frames of w x h"""
    def __init__(self, orc, frames, w=W, h=H):
        self.orc, self.frames, self.lv, self.cache, self.w, self.h = orc, frames, {}, {}, w, h

    def levels(self, g):
        if g not in self.lv:
            pyr = self.orc.half_pyramid(self.frames[g])
            gx, gy = [], []
            for lv in pyr:
                a, b, _ = self.orc.scharr_gradient(lv, 3)
                gx.append(a); gy.append(b)
            self.lv[g] = (pyr, gx, gy)
        return self.lv[g]

    def align(self, j, g, prev_kp):
        key = (j, g, prev_kp.tobytes())
        if key not in self.cache:
            (p0, gx, gy), (p1, _, _) = self.levels(j), self.levels(g)
            cand = [self.orc.patch_points(prev_kp, self.w, self.h, l) for l in range(5)]
            self.cache[key] = self.orc.estimate_pose_features(self.orc.default_align_params(), self.w, self.h, p0, p1, gx, gy, cand)
        return self.cache[key]
