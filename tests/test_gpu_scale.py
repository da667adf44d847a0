"""GPU: size-independent properties at BASELINE.json's full sizes, where the oracle cannot follow (its Gram-space
loop needs hours at C2 and a 20 GB X'X at C3):
  * independent kernels agree: the look-ahead MFMA kernel (complete-data forms of kappa / ELBO) against the masked MFMA
    kernel (NA forms, per-trait Gram blocks; forced by one missing entry in an otherwise identical Y) -- two different
    statements of the same sweep;
  * the ELBO never decreases after the annealing ladder; hotspot counts stay within bounds.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _bench_problem(n, p, q, na_entry=False):
    import bench
    X, Y, lh, li = bench.build_problem(n, p, q, 0, q, 0)
    if na_entry:
        Y = Y.copy()
        Y[7, 3] = np.nan
    return X, Y, lh, li


def _run(X, Y, lh, li, q, sweeps, **env):
    from atlasqtl_amd.core import VbRun
    run = VbRun(Y, X, lh, li, (1, 2, 10), tol=1e-12, maxit=sweeps, thinned_elbo_eval=False, debug=True, device=0, q_total=q)
    run.run()
    st, tr = run.status(), run.elbo_trace()
    rs, nb = run.hotspot_sizes(0.5)
    run.close()
    return st, tr, rs, nb


def test_c2_two_kernels_agree_and_elbo_is_monotone(monkeypatch):
    """C2 = BASELINE.json configs[1]: n = 1000, p = 5000, q = 1000, horseshoe, annealing (1, 2, 10)."""
    n, p, q, sweeps = 1000, 5000, 1000, 40
    X, Y, lh, li = _bench_problem(n, p, q)
    st_a, tr_a, rs_a, nb_a = _run(X, Y, lh, li, q, sweeps)
    assert st_a["core_kernel"] == 0 and st_a["it"] == sweeps
    its, lbs = tr_a
    assert len(lbs) >= 25 and np.all(np.diff(lbs) > -1e-6 * np.abs(lbs[0]) * 1e-6)      # monotone (debug=True also enforces it)
    X2, Y2, lh2, li2 = _bench_problem(n, p, q, na_entry=True)
    st_c, tr_c, rs_c, nb_c = _run(X2, Y2, lh2, li2, q, sweeps)      # look-ahead kernel, MASK instances (per-trait Gram blocks from HBM)
    assert st_c["core_kernel"] == 0
    monkeypatch.setenv("AQ_KERNEL", "3")                            # the two-barrier masked kernel: an independent statement of the NA forms
    st_b, tr_b, rs_b, nb_b = _run(X2, Y2, lh2, li2, q, sweeps)
    assert st_b["core_kernel"] == 3
    np.testing.assert_allclose(tr_c[1], tr_b[1], rtol=1e-10)
    assert nb_c == nb_b
    # one entry of 10^6 is missing: the two runs differ by that entry's information only (~1e-6 relative on the ELBO)
    np.testing.assert_allclose(tr_b[1], tr_a[1], rtol=2e-5)
    assert abs(nb_a - nb_b) <= max(2, nb_a // 100)


def test_c3_sweeps_are_monotone_and_bounded():
    """C3 = BASELINE.json configs[2] (the bench workload): 14 sweeps at full size; ELBO rises on every evaluation after the
    ladder, sweeps/s is of the order bench.py reports, hotspot counts are sane."""
    import time
    n, p, q = 1000, 50000, 10000
    X, Y, lh, li = _bench_problem(n, p, q)
    t0 = time.time()
    st, (its, lbs), rs, nb = _run(X, Y, lh, li, q, 14)
    assert st["it"] == 14 and st["core_kernel"] == 0
    assert len(lbs) >= 3 and np.all(np.diff(lbs) > 0)
    assert rs.shape == (p,) and 0 <= nb <= p * q
    assert st["core_ms"] / st["core_launches"] < 120.0          # ms per core launch; 45 measured


def test_c5_shaped_slice_two_kernels_agree(monkeypatch):
    """C5 = BASELINE.json configs[4] is n = 5000, p = 200 000, q = 20 000 with 5 % of Y missing on 8 GPUs; here a slice of it at
    full n and p (48 of the traits): the look-ahead kernel's MASK instances with the sample split (Gram blocks streamed from
    HBM by LDS-DMA, partial S' exchanged between 3 workgroups per trait tile) against the round-1 masked kernel (Gram
    corrections recomputed per sweep, two barriers per block) -- two independent statements of coreDualMisLoop's sweep, over
    all 12 500 SNP blocks; ELBO monotone after the ladder."""
    n, p, q, sweeps = 5000, 200000, 48, 13
    monkeypatch.setenv("AQ_BENCH_NA", "0.05")
    X, Y, lh, li = _bench_problem(n, p, q)
    assert np.isnan(Y).mean() > 0.03
    st_a, tr_a, rs_a, nb_a = _run(X, Y, lh, li, q, sweeps)
    assert st_a["core_kernel"] == 0 and st_a["it"] == sweeps
    assert np.all(np.diff(tr_a[1][-3:]) > 0)
    monkeypatch.setenv("AQ_KERNEL", "3")
    st_b, tr_b, rs_b, nb_b = _run(X, Y, lh, li, q, sweeps)
    assert st_b["core_kernel"] == 3
    np.testing.assert_allclose(tr_a[1], tr_b[1], rtol=1e-10)
    assert nb_a == nb_b and np.array_equal(rs_a, rs_b)


def _shard_worker(rank, world, port, outdir, n, p, q, sweeps):
    import os
    from tests.util import gloo_rank
    dist = gloo_rank(rank, world, port)
    import bench
    from atlasqtl_amd.core import VbRun
    tiles = (q + 15) // 16
    k0, k1 = min(q, 16 * ((tiles * rank) // world)), min(q, 16 * ((tiles * (rank + 1)) // world))
    X, Y, lh, li = bench.build_problem(n, p, q, k0, k1, 0)
    run = VbRun(Y, X, lh, li, (1, 2, 10), tol=1e-12, maxit=sweeps, thinned_elbo_eval=False, debug=True, device=0, q_total=q,
                process_group=dist.group.WORLD)
    run.run()
    its, lbs = run.elbo_trace()
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), lbs=lbs, it=run.status()["it"])
    run.close()
    dist.destroy_process_group()


def test_c2_two_trait_shards_reproduce_the_single_shard_elbo(tmp_path):
    """The q-sharded protocol at C2 size (two processes share the one GPU, payloads reduced through gloo on the host): same
    ELBO trace as the unsharded run -- the all-reduced sums are added in a different order, nothing else differs."""
    from tests.util import spawn_ranks
    n, p, q, sweeps = 1000, 5000, 1000, 16
    spawn_ranks(_shard_worker, 2, str(tmp_path), n, p, q, sweeps)
    X, Y, lh, li = _bench_problem(n, p, q)
    st, (its, lbs), _, _ = _run(X, Y, lh, li, q, sweeps)
    r0, r1 = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    assert int(r0["it"]) == int(r1["it"]) == st["it"] == sweeps
    np.testing.assert_array_equal(r0["lbs"], r1["lbs"])
    np.testing.assert_allclose(r0["lbs"], lbs, rtol=1e-10)
