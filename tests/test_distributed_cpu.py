"""world_size-2 gloo test (CPU): the q-sharded protocol -- each rank holds half of the traits and
the ranks exchange exactly the payload the HIP path all-reduces (p + 3 doubles per sweep, 6 on ELBO
sweeps) -- reproduces the unsharded run: same iteration count, same ELBO trace, same state."""
import os

import numpy as np
import torch

from tests.util import gloo_rank, make_problem, shard_lists, spawn_ranks


def _worker(rank, world, port, outdir):
    dist = gloo_rank(rank, world, port)
    from oracle import sharded_oracle as S
    prob = make_problem(100, 75, 20, p_act=10, prob_assoc=1.0)
    q = 20
    k0, k1 = (0, 16) if rank == 0 else (16, 20)       # shards are whole 16-trait tiles, as in bench.py
    lh, li = shard_lists(prob["list_hyper"], prob["list_init"], k0, k1)
    calls = []

    def allreduce(v):
        t = torch.from_numpy(np.ascontiguousarray(v))
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        calls.append(t.numel())
        return t.numpy()

    tr = []
    out = S.run_sharded(prob["Y"][:, k0:k1], prob["X"], q, (1, 2, 10), 0.1, 1000, lh, li, allreduce=allreduce, trace=tr)
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), it=out["it"], lb=np.array([r["lb"] for r in tr if r["lb"] is not None]),
             gam=out["gam_vb"], mu=out["mu_beta_vb"], theta=out["theta_vb"], zeta=out["zeta_vb"], calls=np.array(calls))
    dist.destroy_process_group()


def test_q_sharded_protocol_two_ranks(tmp_path):
    from oracle import atlasqtl_oracle as O
    spawn_ranks(_worker, 2, str(tmp_path))
    prob = make_problem(100, 75, 20, p_act=10, prob_assoc=1.0)
    tr = []
    ref = O.atlasqtl_global_local_core_(prob["Y"], prob["X"], 20, (1, 2, 10), 1, 0.1, 1000, prob["list_hyper"],
                                        prob["list_init"], trace=tr, full_output=True)
    r0, r1 = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    assert int(r0["it"]) == int(r1["it"]) == ref["it"]
    lref = np.array([r["lb"] for r in tr if r["lb"] is not None])
    np.testing.assert_allclose(r0["lb"], lref, rtol=1e-10)
    np.testing.assert_array_equal(r0["lb"], r1["lb"])            # every rank assembles the identical ELBO
    np.testing.assert_array_equal(r0["theta"], r1["theta"])      # replicated p-vector state stays identical
    gam = np.concatenate([r0["gam"], r1["gam"]], axis=1)
    mu = np.concatenate([r0["mu"], r1["mu"]], axis=1)
    np.testing.assert_allclose(gam, ref["gam_vb"], atol=1e-9)
    np.testing.assert_allclose(mu, ref["mu_beta_vb"], rtol=1e-7, atol=1e-11)
    np.testing.assert_allclose(np.concatenate([r0["zeta"], r1["zeta"]]), ref["zeta_vb"], rtol=1e-8)
    # payload sizes: p + 3 per sweep (plus the initial one), 8 on ELBO sweeps
    sizes = set(int(x) for x in r0["calls"])
    assert sizes == {prob["p"] + 3, 8}
