"""GPU: bench.py as a program, at a small size (AQ_BENCH_N/P/Q): a plain run times exactly --steps sweeps and prints the
headline line without the --full legs; --dump-outputs writes the VB state of the last timed sweep, the same on every run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, P, Q, STEPS, WARMUP = 100, 300, 40, 3, 10


def _bench(out_dir):
    env = dict(os.environ, AQ_BENCH_N=str(N), AQ_BENCH_P=str(P), AQ_BENCH_Q=str(Q))
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_plain_run_and_dumped_outputs(tmp_path):
    dumps = []
    for i in range(2):
        line = _bench(tmp_path / str(i))
        assert line["steps"] == STEPS and line["warmup"] == WARMUP
        assert line["unit"] == "sweeps/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
        assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(1e3 / line["ms_per_step"])
        assert "cpu_baseline" not in line and "elbo_to_tol" not in line
        files = sorted((tmp_path / str(i)).glob("*.npy"))
        assert sum(f.stat().st_size for f in files) <= 64 << 20
        dumps.append({f.stem: np.load(f) for f in files})
    a, b = dumps
    assert set(a) == {"beta_vb", "gam_vb", "mu_beta_vb", "theta_vb", "zeta_vb", "lam2_inv_vb", "sig2_theta_vb", "tau_vb",
                      "sig2_beta_vb", "it", "lb_opt", "diff_lb", "sig02_inv_vb", "sig2_inv_vb"}
    assert all(v.dtype == np.float64 for v in a.values())
    # until the thinned schedule first evaluates the ELBO, the status has lb_opt = -inf and diff_lb = |-inf - -inf| = NaN
    assert all(np.all(np.isfinite(v)) for k, v in a.items() if k not in ("lb_opt", "diff_lb"))
    for k in ("beta_vb", "gam_vb", "mu_beta_vb"):          # p q is below the sample size: the whole matrix, column-major
        assert a[k].shape == (P * Q,)
    assert a["theta_vb"].shape == (P,) and a["zeta_vb"].shape == (Q,)
    assert np.all((a["gam_vb"] >= 0) & (a["gam_vb"] <= 1))
    np.testing.assert_allclose(a["beta_vb"], a["gam_vb"] * a["mu_beta_vb"], rtol=1e-15, atol=0)
    assert a["it"][0] == WARMUP + STEPS
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
