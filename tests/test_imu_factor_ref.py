"""CPU: the restatement tests/imu_factor_ref.py on the planted motion of tests/vi_align_cases.py (40 chained frames, 200 Hz, integrated deltas).

Measured on the restatement (printed by every run):
  the alignment's own states and EuRoC densities (the scene has no noise, so the states fit the deltas): chi2 of the 38 pairs median 1.2e-6,
    largest 1.7e-6; |r| levels: rotation 2.0e-8 rad, velocity 2.5e-7 m/s, position 1.3e-8 m -- the integrator's and the alignment's own error,
    three orders below the IMU's noise (the first pair has no factor: the root has no velocity under the alignment)
  the planted true states, noisy deltas (30 draws x 39 pairs, seed 20250): mean chi2 8.22, mean chi2_rot 2.90; bands as in test_imu_cov_ref.py (c)
    for N = 1170 and 11 sub-steps a pair: chi2 in [8.09, 9.50], chi2_rot in [2.58, 3.29] (three components: 3 (n - 1/2) / n, sqrt(6 / N))
  one visual rotation turned by 1 degree: chi2_rot of that pair 2.1e5 against at most 4.2e-7 elsewhere"""
import math

import numpy as np
import pytest

import imu_cov_ref as cr
import imu_factor_ref as fr
import imu_ref as ir
import vi_align_cases as vc
import vi_align_ref as vr

N = 40
NOISE = cr.Noise()
DRAWS, SEED = 30, 20250


def planted(n=N, pairing="chain"):
    """the scene, its covariances, the alignment's states and result, and the planted true states with a result that holds the planted gravity"""
    sc = vc.scene(n, pairing, "none", integrate=True)
    delta, cov, _, _ = cr.preintegrate_cov_rows(ir.Params(), NOISE, sc["samples"], sc["times"], sc["prev"], None)
    assert delta.tobytes() == sc["delta"].tobytes()
    state, result, _ = vr.align_rows(sc["P"], sc["prev"], sc["traj"], delta, None)
    true_state = np.zeros(n, vr.STATE_DTYPE)
    for i, t in enumerate(sc["times"]):
        p, v, _ = vc.motion(float(t))
        true_state[i]["p"], true_state[i]["v"], true_state[i]["flags"], true_state[i]["q"] = p, v, vr.VIS_HAS_P | vr.VIS_HAS_V, state[i]["q"]
    true_result = np.zeros(1, vr.RESULT_DTYPE)
    true_result[0]["g"], true_result[0]["s"] = vc.GRAVITY, vc.SCALE
    return dict(sc, cov=cov, state=state, result=np.asarray(result).reshape(1), true_state=true_state, true_result=true_result)


def turned(traj, i, degrees):
    """the trajectory with the rotation of frame i turned about its own z axis, the camera centre kept"""
    out = traj.copy()
    a = math.radians(degrees)
    Rz = [math.cos(a), -math.sin(a), 0.0, math.sin(a), math.cos(a), 0.0, 0.0, 0.0, 1.0]
    R, t = [float(x) for x in traj[i]["R"]], [float(x) for x in traj[i]["t"]]
    C = [-x for x in vr.tmulv(R, t)]
    Rn = ir.mul(Rz, R)
    out[i]["R"], out[i]["t"] = Rn, [-x for x in ir.mulv(Rn, C)]
    return out


def flag_cases(pl):
    """(prev, traj, delta, cov, state, result, FP, {frame: the flags it must have}): every flag reached by a constructed row of the planted call"""
    prev, traj, delta, cov, state = pl["prev"].copy(), pl["traj"].copy(), pl["delta"].copy(), pl["cov"].copy(), pl["true_state"].copy()
    want = {0: fr.IMF_NO_PARENT}                                       # the first frame of a stream
    prev[5], want[5] = ir.KF_NOT_SAVED, fr.IMF_NO_PARENT              # a frame the gate did not save
    prev[6], want[6] = 4, fr.IMF_NO_PARENT                            # its successor pairs with frame 4, but its trajectory record's parent is 5: no edge
    state[9]["flags"] &= ~vr.VIS_HAS_V                                # a frame without a velocity: its own factor and its child's
    want[9], want[10] = fr.IMF_NO_STATE, fr.IMF_NO_STATE
    delta[12]["flags"] |= ir.IMU_GAP                                  # rejected by vp.reject
    cov[13]["flags"] |= cr.IMU_COV_NONFINITE
    cov[14]["q"] = 3
    cov[15]["S"][7] = float("inf")
    delta[16]["dt"] = 0.0
    want.update({12: fr.IMF_UNUSABLE, 13: fr.IMF_UNUSABLE, 14: fr.IMF_UNUSABLE, 15: fr.IMF_UNUSABLE, 16: fr.IMF_UNUSABLE})
    delta[10]["flags"] |= ir.IMU_EMPTY                                # two flags at once
    want[10] |= fr.IMF_UNUSABLE
    cov[18]["S"][:] = 0.0                                             # no pivot
    cov[19]["S"][0] = -cov[19]["S"][0]                                # a negative pivot
    want[18], want[19] = fr.IMF_SINGULAR, fr.IMF_SINGULAR
    state[21]["p"][1], state[22]["p"][1] = -1.7e308, 1.7e308          # p_i - p_b overflows
    want[22] = fr.IMF_NONFINITE
    want[21] = want[23] = fr.IMF_SINGULAR                             # (their finite residuals of 1.7e308: the solve's x overflows, which is a failed solve)
    cov[24]["S"][:] = cov[24]["S"] * 1e-296                           # finite pivots and a finite y of 1e306, a chi-square beyond DBL_MAX
    delta[24]["v"][0] += 2e3
    want[24] = fr.IMF_NONFINITE
    return prev, traj, delta, cov, state, want


@pytest.fixture(scope="module")
def pl():
    return planted()


def test_with_the_alignments_own_states(pl):
    f = fr.factor_rows(pl["P"], fr.FactorParams(), pl["prev"], pl["traj"], pl["delta"], pl["cov"], pl["state"], pl["result"])
    # (the root has no velocity under the alignment -- a velocity needs a delta -- so the first pair has no state to stand on)
    assert int(f[0]["flags"]) == fr.IMF_NO_PARENT and int(f[1]["flags"]) == fr.IMF_NO_STATE and not f[:2]["r"].any() and not f["flags"][2:].any()
    assert (f["q"] == pl["state"]["q"]).all()
    assert np.isfinite(f["chi2"]).all() and (f["chi2"][2:] > 0).all() and (f["chi2_rot"][2:] >= 0).all() and (f["chi2_rot"][2:] <= f["chi2"][2:]).all()
    lv = [float(np.abs(f["r"][2:, 3 * k:3 * k + 3]).max()) for k in range(3)]
    print(f"\nthe alignment's own states: chi2 median {np.median(f['chi2'][2:]):.3g}, largest {f['chi2'].max():.3g}; |r| rotation {lv[0]:.2g} rad, "
          f"velocity {lv[1]:.2g} m/s, position {lv[2]:.2g} m")
    # variances of the visual pose's own error at the level of those residuals bring every chi-square down to the order of its dimension
    wide = fr.factor_rows(pl["P"], fr.FactorParams(lv[0] ** 2, lv[1] ** 2, lv[2] ** 2), pl["prev"], pl["traj"], pl["delta"], pl["cov"], pl["state"], pl["result"])
    assert wide["r"].tobytes() == f["r"].tobytes() and (wide["chi2"][2:] < f["chi2"][2:]).all() and wide["chi2"].max() <= 9.0


def test_with_the_true_states_and_noisy_deltas_the_chi_square_is_calibrated(pl):
    rng = np.random.default_rng(SEED)
    sd = math.sqrt(vc.HZ)
    chi2, rot, ns = [], [], int(pl["delta"][1]["n_steps"])
    for _ in range(DRAWS):
        z = pl["samples"].copy()
        z["w"] += rng.normal(0.0, NOISE.sigma_g * sd, z["w"].shape)
        z["a"] += rng.normal(0.0, NOISE.sigma_a * sd, z["a"].shape)
        delta = ir.preintegrate_rows(ir.Params(), z, pl["times"], pl["prev"], None)[0]
        f = fr.factor_rows(pl["P"], fr.FactorParams(), pl["prev"], pl["traj"], delta, pl["cov"], pl["true_state"], pl["true_result"])
        assert not f["flags"][1:].any()
        chi2 += list(f["chi2"][1:])
        rot += list(f["chi2_rot"][1:])
    n, end = len(chi2), (ns - 0.5) / ns
    m9, m3 = float(np.mean(chi2)), float(np.mean(rot))
    b9, b3 = (9 * end - 4 * math.sqrt(18.0 / n), 9 + 4 * math.sqrt(18.0 / n)), (3 * end - 4 * math.sqrt(6.0 / n), 3 + 4 * math.sqrt(6.0 / n))
    print(f"\ntrue states, noisy deltas, {n} pairs of {ns} sub-steps: mean chi2 {m9:.2f} (band {b9[0]:.2f} - {b9[1]:.2f}), mean chi2_rot {m3:.2f} "
          f"(band {b3[0]:.2f} - {b3[1]:.2f})")
    assert n >= 1000 and b9[0] <= m9 <= b9[1] and b3[0] <= m3 <= b3[1]
    clean = fr.factor_rows(pl["P"], fr.FactorParams(), pl["prev"], pl["traj"], pl["delta"], pl["cov"], pl["true_state"], pl["true_result"])
    assert clean["chi2"].max() < 0.05                                  # the integrator's own error is far below the noise


def test_every_flag_is_reached_and_a_flagged_record_is_zero(pl):
    prev, traj, delta, cov, state, want = flag_cases(pl)
    f = fr.factor_rows(pl["P"], fr.FactorParams(), prev, traj, delta, cov, state, pl["true_result"])
    for i in range(N):
        assert int(f[i]["flags"]) == want.get(i, 0), (i, int(f[i]["flags"]))
        assert bool(f[i]["r"].any() or f[i]["chi2"] or f[i]["chi2_rot"]) == (i not in want), i
    seen = 0
    for v in want.values():
        seen |= v
    assert seen == fr.IMF_NO_PARENT | fr.IMF_NO_STATE | fr.IMF_UNUSABLE | fr.IMF_SINGULAR | fr.IMF_NONFINITE
    bad = pl["true_result"].copy()
    for bit in (vr.VIA_FEW, vr.VIA_SINGULAR, vr.VIA_SCALE):
        bad[0]["flags"] = bit | vr.VIA_GRAVITY_NORM
        g = fr.factor_rows(pl["P"], fr.FactorParams(), prev, traj, delta, cov, state, bad)
        assert all(int(g[i]["flags"]) == (want.get(i, 0) if want.get(i, 0) in (fr.IMF_NO_PARENT,) else (want.get(i, 0) & ~(fr.IMF_SINGULAR | fr.IMF_NONFINITE)) | fr.IMF_NO_ALIGN)
                   for i in range(N)) and not g["r"].any() and not g["chi2"].any()
    bad[0]["flags"] = vr.VIA_GRAVITY_NORM | vr.VIA_GYRO_FEW | vr.VIA_RESTART      # not failures of the linear solve
    g = fr.factor_rows(pl["P"], fr.FactorParams(), prev, traj, delta, cov, state, bad)
    assert g.tobytes() == f.tobytes()
    # a variance on the diagonal makes the zero covariance solvable
    h = fr.factor_rows(pl["P"], fr.FactorParams(1e-8, 1e-6, 1e-8), prev, traj, delta, cov, state, pl["true_result"])
    assert int(h[18]["flags"]) == 0 and h[18]["chi2"] > 0


def test_one_visual_rotation_turned_by_a_degree_stands_out(pl):
    last = N - 1                                                       # (the last frame is nobody's parent: one pair changes)
    f = fr.factor_rows(pl["P"], fr.FactorParams(), pl["prev"], turned(pl["traj"], last, 1.0), pl["delta"], pl["cov"], pl["true_state"], pl["true_result"])
    base = fr.factor_rows(pl["P"], fr.FactorParams(), pl["prev"], pl["traj"], pl["delta"], pl["cov"], pl["true_state"], pl["true_result"])
    assert not f["flags"][1:].any() and f[:last].tobytes() == base[:last].tobytes()
    others = float(f["chi2_rot"][:last].max())
    print(f"\none visual rotation turned by 1 degree: chi2_rot {float(f[last]['chi2_rot']):.3g} against at most {others:.3g} elsewhere")
    assert f[last]["chi2_rot"] > 1e3 * max(others, 3.0) and abs(float(np.linalg.norm(f[last]["r"][:3])) - math.sin(math.radians(1.0))) < 1e-4
