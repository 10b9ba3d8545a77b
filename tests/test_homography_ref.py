"""CPU: the restatement of the homography RANSAC and of the H-or-E decision (tests/homography_ref.py) against an independent solver, on
planted planes, and over the classification table -- the scenes of tests/pose_degenerate_cases.py at m = 40 / 300, noise 0 / 0.3 px,
outliers 0 / 25 %, 200 draws of default_rng(7), E from the oracle's essential_ransac at default parameters.

Measured with this file (the figures DESIGN.md section 4.10 quotes):
  ratio score_h / (score_h + score_e): 0.455 ... 0.502 on the 48 planar cases (minimum: far, M 40, noise 0.3, 25 % outliers),
    0.065 ... 0.323 on the 32 others (maximum: forward, M 300, noise 0, no outliers); nothing is left out, h_ratio = 0.40 separates the
    lists and the paper's 0.45 would sit 0.005 below the smallest planar ratio; the smallest decision margin is 5.5e-2
  planted counts met exactly: 30 / 30 and 225 / 225 on plane and tilted
  restatement against numpy's SVD of the 8 x 9 DLT matrix, over the winners of all 104 cases: largest difference 9.6e-7 (line, M 40:
    three of the four sample points nearly collinear); the restatement against itself with the sample rotated by one place: 1.9e-7
    (line, M 300), so the bound is 1.9e-5; over the 80 classified cases alone the two figures are 1.6e-11 and 1.6e-12
  largest squared transfer residual of a winner on its own sample: 6.4e-10 px^2 with the 2^-20 self-check (its bound: 5.991 * 2^-20 =
    5.7e-6 px^2) and 1.6e-11 px^2 without it -- other winners, and on these scenes none of either kind is far off its sample; what the
    check does here is skip 0 ... 196 of the 200 iterations per case, the near-collinear samples of the line rows that the exact-zero
    tests let through"""
import numpy as np
import pytest

import homography_ref as hr
import pose_degenerate_cases as pdc


@pytest.fixture(scope="module")
def table(orc, vislam):
    """(case -> (record, mask, x1, x2, planted)), computed once"""
    cam, hp, draws = hr.Camera(), hr.default_params(), hr.make_draws(7)
    p = pdc.set_mode(vislam.default_params(), "adaptive")
    out = {}
    for c in hr.table_cases():
        x1, x2, planted = hr.make_rows(*c)
        E = orc.essential_ransac(p, x1, x2)[0]
        rec, mask = hr.homography(cam, hp, x1, x2, draws, E)
        out[c] = (rec, mask, x1, x2, planted)
    return out


def test_restatement_against_svd_on_every_winner(table):
    cam, draws = hr.Camera(), hr.make_draws(7)
    own, svd, res, n = {}, {}, 0.0, 0
    for c, (rec, _, x1, x2, _) in table.items():
        if rec["best_iter"] < 0:
            assert c[0] == "same", c                               # one point repeated: no four distinct points, every iteration degenerate
            continue
        s = hr.winner_sample(cam, x1, x2, draws, int(rec["best_iter"]))
        H, _, ok = hr.solve4(*s)
        assert ok
        assert hr.unit_diff(H, rec["H"]) <= 4 * 2.0 ** -52, c       # the record holds this H, normalised (one division and one square root)
        H2, _, ok2 = hr.solve4(*[v[1:] + v[:1] for v in s])        # the same four correspondences, rotated by one place: another rounding
        assert ok2
        own[c], svd[c] = hr.unit_diff(H, H2), hr.unit_diff(H, hr.dlt_svd(*s))
        res = max(res, hr.transfer_residual_px2(cam, H, s))
        n += 1
    bound = max(1e-12, 100.0 * max(own.values()))
    worst = max(svd, key=svd.get)
    cls = [c for c in own if c[0] not in hr.ROBUST_ONLY]
    print(f"{n} winners: restatement vs SVD max {svd[worst]:.3e} at {worst}; restatement vs itself max {max(own.values()):.3e} at "
          f"{max(own, key=own.get)}; bound {bound:.3e}; classified cases alone {max(svd[c] for c in cls):.3e} / {max(own[c] for c in cls):.3e}; "
          f"largest own-sample residual {res:.3e} px^2")
    assert n == 96
    for c in svd:
        assert svd[c] <= bound, (c, svd[c], bound)
    assert res <= 5.991 * 2.0 ** -20 * (1 + 1e-9)                  # the self-check's own bound, in pixels^2


def test_self_check_residuals_without_it():
    """what the 2^-20 self-check is for: the worst own-sample residual of the winners without it (printed; asserted only with it, above)"""
    cam, hp, draws = hr.Camera(), hr.default_params(), hr.make_draws(7)
    worst, skipped = 0.0, []
    for c in hr.table_cases():
        x1, x2, _ = hr.make_rows(*c)
        live0, cnt0 = hr.iterations(cam, hp, x1, x2, draws, self_check=False)
        live1, _ = hr.iterations(cam, hp, x1, x2, draws)
        assert not (live1 & ~live0).any()
        skipped.append(int((live0 & ~live1).sum()))
        best, _ = hr.pick(live0, cnt0, 200)
        if best >= 0:
            s = hr.winner_sample(cam, x1, x2, draws, best)
            worst = max(worst, hr.transfer_residual_px2(cam, hr.solve4(*s)[0], s))
    print(f"without the self-check: worst own-sample residual {worst:.3e} px^2; iterations it skips per case: {min(skipped)} ... {max(skipped)}")
    assert np.isfinite(worst)


@pytest.mark.parametrize("cls", ["plane", "tilted"])
@pytest.mark.parametrize("m", [40, 300])
def test_planted_planes(table, cls, m):
    """noise 0, 25 % of x2 replaced: every planted correspondence is explained by the true homography to float32 rounding, and 200 draws at
    75 % inliers miss an all-inlier sample with probability (1 - 0.75^4)^200 < 1e-32"""
    rec, mask, _, _, planted = table[(cls, m, 0.0, 0.25)]
    print(f"{cls} M{m}: n_inliers {int(rec['n_inliers'])}, planted {planted}")
    assert planted == m - m // 4
    assert int(rec["n_inliers"]) >= planted and int(mask.sum()) == int(rec["n_inliers"])
    assert mask[m // 4:].all()                                      # the planted ones themselves


def test_classification_table(table):
    hp = hr.default_params()
    left_out = {"H": [], "E": []}
    ratios = {"H": [], "E": []}
    margins = []
    for c, (rec, _, _, _, _) in table.items():
        if c[0] in hr.ROBUST_ONLY:
            assert int(rec["model"]) in (0, 1, 2) and np.isfinite(rec["H"]).all() and np.isfinite([rec["score_h"], rec["score_e"]]).all(), c
            continue
        lst = "H" if c[0] in hr.H_LIST else "E"
        assert lst == "H" or c[0] in hr.E_LIST
        r, mg = hr.ratio(rec), hr.margin(rec, hp)
        ratios[lst].append((r, c))
        margins.append((mg, c))
        assert mg > 1e-9, (c, mg)                                  # no decision on a rounding
        if hp.h_ratio - 0.05 <= r <= hp.h_ratio + 0.02:
            left_out[lst].append(c)
            continue
        assert int(rec["model"]) == (hr.MODEL_HOMOGRAPHY if lst == "H" else hr.MODEL_ESSENTIAL), (c, r, rec)
    for k in ("H", "E"):
        print(f"{k} list: ratio {min(ratios[k])[0]:.3f} {min(ratios[k])[1]} ... {max(ratios[k])[0]:.3f} {max(ratios[k])[1]}; left out {left_out[k]}")
    print(f"smallest decision margin {min(margins)[0]:.3e} {min(margins)[1]}")
    assert len(ratios["H"]) == 48 and len(ratios["E"]) == 32
    assert len(left_out["H"]) <= 2 and not left_out["E"]


def test_empty_and_degenerate_rows():
    cam, hp, draws = hr.Camera(), hr.default_params(), hr.make_draws(7)
    x1, x2, _ = hr.make_rows("general", 40, 0.0, 0.0)
    for m in (0, 3):
        rec, mask = hr.homography(cam, hp, x1[:m], x2[:m], draws, np.eye(3))
        assert rec.tobytes() == hr.zero_record().tobytes() and len(mask) == m and not mask.any()
    hp.iters = 0
    assert hr.homography(cam, hp, x1, x2, draws)[0].tobytes() == hr.zero_record().tobytes()
    hp.iters = 200
    # a zero and a NaN E score nothing and are not offered; no E at all gives the same record
    base = hr.homography(cam, hp, x1, x2, draws)[0]
    for E in (np.zeros((3, 3)), np.full((3, 3), np.nan)):
        rec = hr.homography(cam, hp, x1, x2, draws, E)[0]
        assert rec.tobytes() == base.tobytes() and rec["score_e"] == 0.0 and rec["n_inliers_e"] == 0
    # the sign: det >= 0 and unit norm on every winner of a few rows
    for cls in ("general", "plane", "rot", "forward"):
        a, b, _ = hr.make_rows(cls, 40, 0.3, 0.25)
        H = hr.homography(cam, hp, a, b, draws)[0]["H"].reshape(3, 3)
        assert abs(np.linalg.norm(H) - 1.0) <= 4 * 2.0 ** -52 and np.linalg.det(H) > 0
