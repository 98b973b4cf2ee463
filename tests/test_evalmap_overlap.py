"""erasor_amd.evalmap.overlap / overlap_lines (the estimate-to-ground-truth distance report, scripts/analysis_runner.py:53-71) against
the reference's own overlap_report: tests/golden/overlap_golden.npz holds its captured stdout and the exact numbers of its calls
(tests/golden/make_overlap_golden.py)."""
import os

import numpy as np

from erasor_amd import evalmap

HERE = os.path.dirname(os.path.abspath(__file__))


def golden():
    z = np.load(os.path.join(HERE, "golden", "overlap_golden.npz"))
    fields = [str(f) for f in z["fields"]]
    for k in range(int(z["n_cases"])):
        yield str(z["name%d" % k]), z["gt%d" % k], z["est%d" % k], float(z["vs%d" % k]), dict(zip(fields, z["res%d" % k].tolist())), \
            str(z["text%d" % k])


def same_bits(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def test_overlap_reproduces_the_reference_numbers_bit_for_bit():
    n = 0
    for name, gt, est, vs, want, _ in golden():
        r = evalmap.overlap(gt[:, :3], est[:, :3], vs)
        for k, v in want.items():
            assert same_bits(r[k], v), (name, k, r[k], v)
        n += 1
    assert n == 8


def test_overlap_lines_reproduce_the_reference_text():
    for name, gt, est, vs, _, text in golden():
        r = evalmap.overlap(gt[:, :3], est[:, :3], vs)
        assert "\n".join(evalmap.overlap_lines(r, vs)) + "\n" == text, name


def test_golden_cases_cover_the_pitfalls():
    cases = {name: (gt, est, want) for name, gt, est, _, want, _ in golden()}
    assert cases["misaligned_0.35m_1.5deg"][2]["frac_half"] < 10.0 < cases["aligned_3cm"][2]["frac_half"]
    assert cases["outliers_1pct"][2]["max"] > 50.0
    assert cases["duplicates_and_exact_hits"][2]["n_below_half"] > 0
    assert np.all(cases["planar_gt"][0][:, 2] == 0)
    assert cases["single_estimate"][2]["n_est"] == 1
    assert {int(w["n_est"]) % 2 for _, _, w in cases.values()} == {0, 1}
    assert np.abs(cases["utm_scale"][0][:, :2]).min() > 3e5


def test_empty_estimate_gives_nan_statistics():
    r = evalmap.overlap(np.zeros((3, 3), np.float32), np.zeros((0, 3), np.float32), 0.2)
    assert r["n_est"] == 0 and r["n_below_two"] == 0 and np.isnan(r["median"]) and np.isnan(r["frac_one"])
