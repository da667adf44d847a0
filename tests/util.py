"""Shared problem builders for the test-suite (inputs only; no oracle logic here)."""
import numpy as np

from atlasqtl_amd import hyper_init as H
from atlasqtl_amd import synth
from oracle import prepare_oracle


def shard_lists(list_hyper, list_init, k0, k1):
    """Copies of the two argument lists for the trait shard [k0, k1): the q-indexed vectors and the columns of the two
    p x q initial matrices (left alone when they are None: drawn on the device)."""
    lh, li = dict(list_hyper), dict(list_init)
    for k in ("eta", "kappa", "n0"):
        lh[k] = np.asarray(lh[k])[k0:k1]
    for k in ("sig2_beta_vb", "tau_vb", "zeta_vb"):
        li[k] = np.asarray(li[k])[k0:k1]
    for k in ("gam_vb", "mu_beta_vb"):
        if li.get(k) is not None:
            li[k] = np.asarray(li[k])[:, k0:k1]
    return lh, li


def gloo_rank(rank, world, port, backend="gloo"):
    """The prologue of a spawned worker: the repository on sys.path and this process in a group of `world` ranks (gloo unless
    another backend is named).  Returns torch.distributed (the worker ends with its destroy_process_group())."""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group(backend, rank=rank, world_size=world)
    return dist


def spawn_ranks(worker, world, *args):
    """Run worker(rank, world, port, *args) in `world` processes (worker: a module-level function, spawn pickles it by
    name) on a free local port, and wait for them."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(worker, args=(world, port) + args, nprocs=world, join=True)


def make_problem(n, p, q, p_act=10, seed=123, init_seed=456, maf=0.2, p0=(5, 25), prob_assoc=0.2, na_frac=0.0,
                 q_act=None):
    """Synthetic data in the shape of the reference's example generator, pre-processed by the
    host mirror of prepare_data_, with automatic hyper-parameters and a seeded automatic init."""
    d = synth.simulate(n, p, q, p_act=p_act, q_act=q_act, seed=seed, maf=maf, prob_assoc=prob_assoc, na_frac=na_frac)
    # host arrays for both sides of a parity test: the NumPy restatement of prepare_data_ (the device-side preparation has
    # its own tests against it, tests/test_gpu_prepare.py)
    X, Y, bool_cst, bool_coll = prepare_oracle.prepare_xy(d["Y"], d["X"])
    bool_rmvd_x = bool_cst.copy()
    bool_rmvd_x[~bool_cst] = bool_coll
    pp = X.shape[1]
    lh = H.prepare_list_hyper_(None, Y, pp, p0, bool_rmvd_x)
    li = H.prepare_list_init_(None, Y, pp, p0, bool_rmvd_x, q, init_seed)
    return dict(X=X, Y=Y, list_hyper=lh, list_init=li, truth=d, n=n, p=pp, q=q)


# ------------------------------------------------------------------------------------------------------------------------------
# Inputs of the trait-sharded runs (tests/test_shard_coverage_host.py asserts what they hold, tests/test_gpu_shard_schemes.py
# runs them).
SHARD_HETERO_SHAPE = (1300, 70, 48)
SHARD_HETERO_NA = (16, 32, 0.05)            # traits [16, 32) lose 5 % of their samples
SHARD_HETERO_TRAIT = (37, 1030)             # trait 37 loses 1030 of its 1300: more than AQ_MIS_MMAX = 1024
SHARD_SMALL_Q = (17, 33, 40)


def make_shard_problem(kind, q=None, na=0.0):
    """kind = "hetero": make_problem(1300, 70, 48) whose three 16-trait shards fall to three kernel families -- traits [0, 16)
    complete (look-ahead kernel), [16, 32) with 5 % NaN (its MASK instance), and trait 37 with 1030 missing samples, which hands
    the whole shard [32, 48) to the generic kernel; every column re-centred over its observed rows.  The lists are those of the
    complete problem.  kind = "small": make_problem(300, 70, q) with q in SHARD_SMALL_Q and na = 0 or 0.04 sprinkled uniformly."""
    if kind == "small":
        if q not in SHARD_SMALL_Q or na not in (0.0, 0.04):
            raise ValueError("make_shard_problem: 'small' takes q in (17, 33, 40) and na in (0, 0.04)")
        return make_problem(300, 70, q, p_act=8, prob_assoc=0.3, seed=123, na_frac=na)
    if kind != "hetero" or q is not None or na:
        raise ValueError("make_shard_problem: kind is 'hetero' (no further argument) or 'small'")
    n, p, q = SHARD_HETERO_SHAPE
    prob = make_problem(n, p, q, p_act=8, prob_assoc=0.3, seed=123)
    rng = np.random.default_rng(9)
    Y = np.array(prob["Y"], dtype=np.float64, order="F")
    k0, k1, frac = SHARD_HETERO_NA
    Y[:, k0:k1][rng.random((n, k1 - k0)) < frac] = np.nan
    k, m = SHARD_HETERO_TRAIT
    Y[rng.choice(n, size=m, replace=False), k] = np.nan
    prob["Y"] = np.asfortranarray(Y - np.nanmean(Y, axis=0)[None, :])
    return prob


# ------------------------------------------------------------------------------------------------------------------------------
# Inputs that drive the probit link u = theta_j + zeta_k over its whole domain (tests/test_link_coverage_host.py asserts what
# they cover, tests/test_gpu_link_range.py runs them).  The constants restate atlasqtl_amd/csrc/aq_probit_tab.h.
LINK_W, LINK_NI, LINK_R = 0.5, 24, 12.0     # AQ_PT_W, AQ_PT_NI, AQ_PT_R: 24 intervals of width 1/2 on |u| < 12, a series beyond
LINK_GROUP = 16                             # a helper wave stages 16 SNPs x 16 traits: the wave votes on "all lanes in the tables"
LINK_EDGES = (0.5, 3.0, 6.5, 11.5, 12.0)    # interval boundaries that also get their two floating-point neighbours, on both signs


def _link_coarse(m, spread, fine):
    """m values in +-spread in groups of LINK_GROUP: groups whose every |value| <= 12 - fine - 1/16 (with a fine part in +-fine
    every u is inside the tables, up to |u| = 12 - 1/16), groups that hold values on both sides of |u| = 12, groups whose every |value| >= 14, and the ragged
    rest inside.  Neighbours inside the tables, and in the tail up to |u| = 21, are at most 2 fine apart, so that with the fine
    part u leaves no gap there (21 = 12 / sqrt(1/3): sqrt(c) u of the ladders in use still meets every interval).  All values
    are multiples of 1/64, so that value + fine part is exact."""
    if spread < 14.0:
        raise ValueError("make_link_problem: spread must be at least 14 (the tail groups start there)")
    full = m // LINK_GROUP
    if full < 3:
        raise ValueError("make_link_problem: the spread axis needs at least three full groups of 16")
    n_mix, n_out = max(1, full // 4), max(1, (full + 1) // 3)
    n_in = m - LINK_GROUP * (n_out + n_mix)
    n_neg = (3 * n_in + 2) // 5                       # the negative side gets the denser grid: A is odd, and gam_vb saturates at 1
    top = LINK_R - fine - 1.0 / 16.0                   # an all-inside wave reaches |u| = 12 - 1/16: the last interval's upper half
    inside = np.concatenate([[-top], np.linspace(-10.5, -0.5, n_neg - 1), np.linspace(0.0, 10.0, n_in - n_neg - 1), [top]])
    mixed = np.array([-13.0, -12.5, -12.0, -11.5, -11.0, 11.0, 11.5, 12.0, 12.5, 13.0, -6.25, -2.75, 3.5, -8.75, -12.25, -11.75])
    mixed = np.concatenate([mixed + g / 16.0 * np.sign(mixed) * (np.abs(mixed) < 11.0) for g in range(n_mix)])
    nt = 8 * n_out
    near = np.arange(14.0, 21.0 + 2.0 * fine, 2.0 * fine)
    if spread >= near[-1] + 3.0 and nt >= near.size + 3:
        mag = np.concatenate([near, np.linspace(near[-1] + 2.0, spread, nt - near.size)])
    else:
        mag = np.linspace(14.0, spread, nt)
    tail = np.concatenate([np.concatenate([-mag[g::n_out], mag[g::n_out]]) for g in range(n_out)])
    ragged = m - LINK_GROUP * full
    v = np.concatenate([inside[:n_in - ragged], mixed, tail, inside[n_in - ragged:]])
    assert v.size == m
    v = np.round(v * 64.0) / 64.0
    if np.max(np.diff(np.sort(v[np.abs(v) <= LINK_R]))) > 2.0 * fine:
        raise ValueError("make_link_problem: too few entries on the spread axis to cover the tables with this fine range")
    return v


def _link_fine(m, coarse, fine, rng):
    """m values in [-fine, fine]: the differences that put u exactly on every interval boundary k/2 (0 and +-12 among them) and
    on the two floating-point neighbours of +-LINK_EDGES (so nextafter(+-12, 0) too), a dyadic grid, and seeded multiples
    of 2^-10; shuffled, so that the special values are spread over the SNP blocks / trait tiles."""
    targets = [k * LINK_W for k in range(-LINK_NI, LINK_NI + 1)]
    targets += [np.nextafter(s * e, toward) for e in LINK_EDGES for s in (-1.0, 1.0) for toward in (-np.inf, np.inf)]
    special = []
    for t in targets:
        c = coarse[np.argmin(np.abs(coarse - t))]
        f = t - c
        if abs(f) > fine or f + c != t:
            raise ValueError(f"make_link_problem: cannot place u = {t!r} exactly")
        special.append(f)
    left = m - len(special)
    step = next((s for s in (32, 16, 8, 4) if 2 * s + 1 <= left), None)
    if step is None:
        raise ValueError(f"make_link_problem: the fine axis needs at least {len(special) + 9} entries")
    grid = np.arange(-step, step + 1) / float(step) * fine
    rest = np.round(rng.integers(-1024, 1025, size=left - grid.size) * fine) / 1024.0
    v = np.concatenate([special, grid, rest])
    return v[rng.permutation(m)]


def make_link_problem(n, p, q, spread_axis="zeta", spread=38.0, fine=0.5, fine_scale=1.0, link_seed=7, **kw):
    """make_problem(n, p, q, **kw) with list_init["theta_vb"] and list_init["zeta_vb"] -- and nothing else -- replaced, so that
    u = theta_j + zeta_k covers the whole domain of the probit link: every one of the 24 table intervals on both signs, the
    boundaries k/2 exactly, +-12 and their neighbours, u = 0, and both tails out to +-(spread + fine).  spread_axis = "zeta":
    the spread is in zeta (trait tiles of 16: inside the tables / mixed / outside) and |theta_j| <= fine, which the annealed
    horseshoe update of the oracle needs; "theta": the spread is in theta (SNP blocks of 16) and
    |zeta_k| <= fine.  fine_scale < 1 shrinks the fine part after it is laid out, for the drivers whose reference formulas
    need a still smaller |theta_j|: u then misses most of the exact boundaries and leaves gaps between neighbours (what it
    still covers is asserted case by case in tests/test_link_coverage_host.py)."""
    if spread_axis not in ("zeta", "theta"):
        raise ValueError("spread_axis must be 'zeta' or 'theta'")
    prob = make_problem(n, p, q, **kw)
    rng = np.random.default_rng(link_seed)
    m_coarse, m_fine = (q, prob["p"]) if spread_axis == "zeta" else (prob["p"], q)
    coarse = _link_coarse(m_coarse, float(spread), float(fine))
    small = _link_fine(m_fine, coarse, float(fine), rng) * float(fine_scale)
    li = dict(prob["list_init"])
    li["zeta_vb"], li["theta_vb"] = (coarse, small) if spread_axis == "zeta" else (small, coarse)
    prob["list_init"] = li
    prob["spread_axis"] = spread_axis
    return prob


def link_interval(x):
    """Signed index of the table interval that holds x: +-(1 + floor(2 |x|)) for |x| < 12, +-(LINK_NI + 1) for the tails, 0 for
    x = 0 exactly -- locate() of aq_core_sweep_la.h, by sign."""
    x = np.asarray(x, dtype=np.float64)
    i = np.minimum(np.floor(np.abs(x) / LINK_W), LINK_NI).astype(np.int64) + 1
    return np.where(x == 0.0, 0, np.sign(x).astype(np.int64) * i)


def link_wave_classes(theta, zeta, sqrt_c=1.0):
    """The vote of every helper wave (SNP block x trait tile): 0 = every lane inside the tables, 1 = mixed, 2 = every lane
    outside.  Returns the (blocks x tiles) array."""
    u = theta[:, None] + zeta[None, :]
    inr = (np.abs(u) < LINK_R) & (np.abs(sqrt_c * u) < LINK_R)
    nb, nt = -(-u.shape[0] // LINK_GROUP), -(-u.shape[1] // LINK_GROUP)
    out = np.empty((nb, nt), dtype=np.int64)
    for b in range(nb):
        for t in range(nt):
            w = inr[LINK_GROUP * b:LINK_GROUP * (b + 1), LINK_GROUP * t:LINK_GROUP * (t + 1)]
            out[b, t] = 0 if w.all() else (2 if not w.any() else 1)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# Inputs along the axes that make_problem never leaves: the Gram structure of X (linkage disequilibrium), the per-entry
# X_norm_sq(j, k) (rare variants whose carriers are missing in a trait), the per-trait scale, and per-trait hyper-parameters
# (tests/test_regime_coverage_host.py asserts what they hold, tests/test_gpu_regimes.py runs them).
REGIMES = ("ld", "rare", "scale")
REGIME_BLOCK = 16                           # SNPs per block of the sweep kernels, traits per trait tile
RARE_STEP, RARE_FIRST = 5, 4                # the rare columns: 4, 9, 14, ...: column 79 is the last of block 4, and the borders
                                            # 16, 32, 48, 96, 112, 128 keep both of their columns for the LD pairs
LD_RHO = (0.002, 0.2)                       # per-SNP flip probabilities of the haplotype copying, log-uniform
LD_BORDER_RHO = 0.002                       # the first SNP of every block copies its neighbour at the lower end: r^2 about 0.99


def block_borders(p):
    """First columns of the SNP blocks 1, 2, ...: a border lies between columns c - 1 and c."""
    return list(range(REGIME_BLOCK, p, REGIME_BLOCK))


def chain_borders(p, nseg):
    """First columns of the chained segments 1 ... nseg - 1 (aq_core_sweep_la.h: segment s starts at block nb s / nseg)."""
    nb = -(-p // REGIME_BLOCK)
    return [REGIME_BLOCK * (nb * s // nseg) for s in range(1, nseg)]


def rare_columns(p):
    return list(range(RARE_FIRST, p, RARE_STEP))


def r2_pair(X, i, j):
    """Squared correlation of two columns."""
    a, b = X[:, i] - X[:, i].mean(), X[:, j] - X[:, j].mean()
    return float((a @ b) ** 2 / ((a @ a) * (b @ b)))


def _regime_genotypes(n, p, regime, rng):
    """n x p dosages and the rare columns with their carriers {column: rows}."""
    from tests.ld_util import haplotype_copy_genotypes
    if "ld" in regime:
        rho = np.exp(rng.uniform(np.log(LD_RHO[0]), np.log(LD_RHO[1]), size=p))
        rho[block_borders(p)] = LD_BORDER_RHO
        G = haplotype_copy_genotypes(n, p, rng, rho, maf=0.3).astype(np.float64)
    else:
        G = rng.binomial(2, 0.2, size=(n, p)).astype(np.float64)
    carriers = {}
    if "rare" in regime:
        cols = rare_columns(p)
        rows = rng.permutation(n)                   # disjoint carriers: no two rare columns are copies of each other
        if 3 * len(cols) > n:
            raise ValueError("make_regime_problem: n is too small for disjoint carriers")
        for i, j in enumerate(cols):
            m = 1 + i % 3                           # 1, 2 or 3 heterozygous carriers
            carriers[j] = np.sort(rows[3 * i:3 * i + m])
            G[:, j] = 0.0
            G[carriers[j], j] = 1.0
    # a column that came out constant or as a copy of an earlier one is drawn again (prepare_xy would drop it and shift the
    # block borders).  In LD that is the usual fate of a SNP with a small flip probability at small n: it is redrawn as its left
    # neighbour with two samples' dosages changed by one, which keeps the link; otherwise independently
    for _ in range(100):
        Xs = prepare_oracle.scale_columns(G)
        bad = [j for j in range(p) if not np.all(np.isfinite(Xs[:, j]))]
        seen = {}
        for j in range(p):
            if j not in bad and seen.setdefault(Xs[:, j].tobytes(), j) != j:
                bad.append(j)
        if not bad:
            return G, carriers
        for j in sorted(bad):
            if j in carriers:
                raise ValueError("make_regime_problem: a rare column is a copy")
            if "ld" in regime and j > 0 and j - 1 not in carriers:
                G[:, j] = G[:, j - 1]
                rows = rng.choice(n, size=2, replace=False)
                G[rows, j] = np.where(G[rows, j] < 2.0, G[rows, j] + 1.0, 1.0)
            else:
                G[:, j] = rng.binomial(2, 0.3, size=n)
    raise ValueError("make_regime_problem: cannot draw distinct columns")


def regime_scales(q, rng):
    """s_k of Y[:, k] *= 10^s_k: uniform in [-4, 4], with both ends next to each other in the first trait tile and in the
    last (ragged) one."""
    s = rng.uniform(-4.0, 4.0, size=q)
    t_last = REGIME_BLOCK * ((q - 1) // REGIME_BLOCK)
    if q - t_last < 2 or t_last == 0:
        raise ValueError("make_regime_problem: q needs a full trait tile and a last tile of at least two traits")
    s[1], s[14] = -4.0, 4.0
    s[q - 2], s[q - 1] = 4.0, -4.0
    return s


def make_regime_problem(n, p, q, regime, na_frac=0.0, hyper="auto", seed=31, init_seed=456, p0=(5, 25)):
    """A problem in the form of make_problem whose inputs leave what make_problem always gives (independent common SNPs, traits
    of variance about 1, hyper-parameters and init constant over the traits).  regime: a set of
      "ld"     genotypes from haplotype copying with per-SNP flip probabilities in LD_RHO; the first SNP of every 16-SNP block
               copies its left neighbour with LD_BORDER_RHO, so r^2 >= 0.95 straddles the block borders (and every border of
               chained segments, which are block borders); the active SNPs include such a pair, 47 and 48;
      "rare"   every 5th column (4, 9, ...) has 1, 2 or 3 heterozygous carriers; column 79 is the last of its block; with
               na_frac > 0 all carriers of three of them -- 79 among them -- are missing in one trait each, the traits in
               different trait tiles (as far as q has tiles);
      "scale"  Y[:, k] *= 10^s_k, s_k from regime_scales.
    hyper = "per_trait": set_hyper with eta_k ~ U(0.5, 20), kappa_k = v_k U(0.2, 5) (v_k: the trait's variance), n0_k = the
    automatic n0 + U(-1.5, 1.5), nu = 0.5, rho = 3, t02 = 2.5 x the automatic one, and list_init["tau_vb"] = U(0.5, 2) / v_k:
    every q-vector distinct in every entry.  Extra keys of the result: carriers, dropped = [(SNP, trait)], active, scales."""
    regime = frozenset(regime)
    if not regime <= set(REGIMES):
        raise ValueError(f"regime must be a subset of {REGIMES}")
    if hyper not in ("auto", "per_trait"):
        raise ValueError("hyper must be 'auto' or 'per_trait'")
    if p <= 80:
        raise ValueError("make_regime_problem: p must exceed 80 (the rare column 79, the active pair 47 / 48)")
    rng = np.random.default_rng(seed)
    G, carriers = _regime_genotypes(n, p, regime, rng)
    # effects: the neighbours 47 and 48 (in LD they share their signal, across a block border), a rare SNP, and five others
    others = [j for j in rng.permutation(p) if j not in (47, 48, 79) and j not in carriers][:5]
    active = np.sort(np.array([47, 48, 79 if "rare" in regime else 80] + others))
    sub = rng.random((active.size, q)) < 0.3
    beta = np.where(sub, rng.normal(size=sub.shape), 0.0)
    Gs = (G - G.mean(0)) / G.std(0, ddof=1)
    Y = rng.normal(size=(n, q)) + Gs[:, active] @ (beta * 0.5)
    scales = regime_scales(q, rng) if "scale" in regime else np.zeros(q)
    Y = Y * 10.0 ** scales[None, :]
    dropped = []
    if na_frac > 0:
        Y[rng.random((n, q)) < na_frac] = np.nan
        if "rare" in regime:
            nt = -(-q // REGIME_BLOCK)
            snps = [79] + [j for j in sorted(carriers) if len(carriers[j]) == 3 and j != 79][:2]
            for i, j in enumerate(snps):
                k = min(q - 1, REGIME_BLOCK * (i % nt) + 3 + i)
                Y[carriers[j], k] = np.nan
                dropped.append((j, k))
    X, Yc, bool_cst, bool_coll = prepare_oracle.prepare_xy(Y, G)
    bool_rmvd_x = bool_cst.copy()
    bool_rmvd_x[~bool_cst] = bool_coll
    pp = X.shape[1]
    auto = H.auto_set_hyper_(Yc, pp, p0)
    li = H.prepare_list_init_(None, Yc, pp, p0, bool_rmvd_x, q, init_seed)
    if hyper == "per_trait":
        v = np.nanvar(Yc, axis=0, ddof=1)
        hr = np.random.default_rng(seed + 1000)
        lh = H.set_hyper(q, p, eta=hr.uniform(0.5, 20.0, size=q), kappa=v * hr.uniform(0.2, 5.0, size=q),
                         n0=auto["n0"] + hr.uniform(-1.5, 1.5, size=q), nu=0.5, rho=3.0, t02=2.5 * auto["t02"])
        lh = H.prepare_list_hyper_(lh, Yc, pp, p0, bool_rmvd_x)
        li = H.ListInit(li)
        li.cls = "out_init"
        li["tau_vb"] = hr.uniform(0.5, 2.0, size=q) / v
    else:
        lh = H.prepare_list_hyper_(None, Yc, pp, p0, bool_rmvd_x)
    return dict(X=X, Y=Yc, list_hyper=lh, list_init=li, truth=dict(X=G, Y=Y, beta=beta), n=n, p=pp, q=q, p_drawn=p,
                carriers=carriers, dropped=dropped, active=active, scales=scales, regime=regime, hyper=hyper)


# ------------------------------------------------------------------------------------------------------------------------------
# Inputs for the p- and q-vector kernels at the edges of their launch grids (tests/test_vector_coverage_host.py asserts what they
# hold, tests/test_gpu_vector_edges.py runs them).
VECTOR_SCALE = 4.0                          # Y[:, k] *= 10^s_k with s_k in [-4, 4], as regime_scales
VECTOR_BORDER_TRAITS = (255, 256, 1023, 1024, 2047, 2048)      # blocks of 256 q-threads, strides of 1024


def theta_for_L(list_init, q, positions, L, df=1):
    """theta_vb values at `positions` that make the first sweep without annealing compute L_j = sig02_inv_vb shr (theta_j^2 +
    sig2_theta_j) / (2 df) (R/atlasqtl_global_local_core.R:241 with m0 = 0, shr = q) equal to L; the signs alternate."""
    positions = np.asarray(positions, dtype=np.int64)
    L = np.broadcast_to(np.asarray(L, dtype=np.float64), positions.shape)
    t2 = 2.0 * df * L / (float(list_init["sig02_inv_vb"]) * q) - np.asarray(list_init["sig2_theta_vb"])[positions]
    if np.any(t2 < 0):
        raise ValueError("theta_for_L: an L below the one theta_j = 0 gives")
    return np.sqrt(t2) * np.where(positions % 2 == 0, 1.0, -1.0)


def make_vector_problem(n, p, q, na_frac=0.0, theta=None, df=1, seed=123, hyper_seed=1031, init_seed=456, p0=(5, 25)):
    """A problem in the form of make_problem in which every trait differs from its neighbours in every q-vector a kernel reads,
    so that a trait index that slips by one across a thread-block or stride border changes a number a test reads: the data of
    make_problem(n, p, q, p_act=8, prob_assoc=0.3, na_frac=na_frac, seed=seed) with Y[:, k] *= 10^s_k, s_k ~ U(-4, 4), and the
    per-trait hyper-parameters and initial tau_vb of make_regime_problem(..., {"scale"}, hyper="per_trait"): eta_k ~ U(0.5, 20),
    kappa_k = v_k U(0.2, 5), n0_k = the automatic n0 + U(-1.5, 1.5), nu = 0.5, rho = 3, t02 = 2.5 x the automatic one, tau_vb =
    U(0.5, 2) / v_k.  (One builder for every p and q: regime_scales refuses q = 16 m + 1, make_regime_problem p <= 80.)  The
    traits VECTOR_BORDER_TRAITS and the last two are associated with all eight active SNPs and have n0_k at the upper end.
    theta: None, or (positions, L): list_init["theta_vb"] -- and nothing else -- is replaced at those predictors by
    theta_for_L(..., df).  Extra keys: scales, theta_positions."""
    d = synth.simulate(n, p, q, p_act=8, seed=seed, maf=0.2, prob_assoc=0.3, na_frac=na_frac)
    hr = np.random.default_rng(hyper_seed)
    scales = hr.uniform(-VECTOR_SCALE, VECTOR_SCALE, size=q)
    border = [k for k in VECTOR_BORDER_TRAITS + (q - 2, q - 1) if 0 <= k < q]
    # the traits on either side of a block or stride border of the q-threads, and the last two, are associated with every active
    # SNP, and (below) get the upper end of n0, each its own value: their columns of gam_vb carry an above-average share of the
    # sums over traits, so a sum that stops one trait short is short by a share that shows
    signs = np.where(np.arange(d["act_x"].size) % 2 == 0, 1.0, -1.0)
    d["Y"][:, border] += (d["X"][:, d["act_x"]] @ signs)[:, None]
    X, Y, bool_cst, bool_coll = prepare_oracle.prepare_xy(d["Y"] * 10.0 ** scales[None, :], d["X"])
    bool_rmvd_x = bool_cst.copy()
    bool_rmvd_x[~bool_cst] = bool_coll
    pp = X.shape[1]
    auto = H.auto_set_hyper_(Y, pp, p0)
    v = np.nanvar(Y, axis=0, ddof=1)
    eta, kappa, shift = hr.uniform(0.5, 20.0, size=q), v * hr.uniform(0.2, 5.0, size=q), hr.uniform(-1.5, 1.5, size=q)
    for i, k in enumerate(border):
        shift[k] = 1.5 - 0.01 * i
    lh = H.set_hyper(q, p, eta=eta, kappa=kappa, n0=auto["n0"] + shift, nu=0.5, rho=3.0, t02=2.5 * auto["t02"])
    lh = H.prepare_list_hyper_(lh, Y, pp, p0, bool_rmvd_x)
    li = H.ListInit(H.prepare_list_init_(None, Y, pp, p0, bool_rmvd_x, q, init_seed))
    li.cls = "out_init"
    li["tau_vb"] = hr.uniform(0.5, 2.0, size=q) / v
    positions = np.zeros(0, dtype=np.int64)
    if theta is not None:
        positions = np.asarray(theta[0], dtype=np.int64)
        th = np.array(li["theta_vb"], dtype=np.float64)
        th[positions] = theta_for_L(li, q, positions, theta[1], df)
        li["theta_vb"] = th
    return dict(X=X, Y=Y, list_hyper=lh, list_init=li, truth=d, n=n, p=pp, q=q, scales=scales, theta_positions=positions)


def operator_inputs(p, q, n=60, seed=0, mis=False, c=1.0):
    """Random but well-formed inputs of coreDualLoop / coreDualMisLoop (R layout)."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, p))
    X = (X - X.mean(0)) / X.std(0, ddof=1)
    Y = rng.normal(size=(n, q))
    gam = np.asfortranarray(rng.uniform(0.01, 0.6, size=(p, q)))
    mu = np.asfortranarray(rng.normal(size=(p, q)) * 0.3)
    m1 = np.asfortranarray(gam * mu)
    theta = rng.normal(size=p) * 0.5
    zeta = rng.normal(size=q) * 0.5 - 1.5
    from scipy.special import log_ndtr
    tz = theta[:, None] + zeta[None, :]
    lP = np.asfortranarray(log_ndtr(tz))
    l1 = np.asfortranarray(log_ndtr(-tz))
    tau = rng.uniform(0.5, 2.0, size=q)
    log_tau = np.log(tau) - 0.01
    out = dict(gam_vb=gam, mu_beta_vb=mu, m1_beta=m1, log_Phi=lP, log_1mPhi=l1, tau_vb=tau, log_tau_vb=log_tau,
               log_sig2_inv_vb=-0.3, c=c, shuffled_ind=np.arange(p, dtype=np.int32),
               sample_q=np.arange(q, dtype=np.int32), X=X, Y=Y)
    if mis:
        mis_pat = (rng.random((n, q)) > 0.1).astype(np.float64)
        Y0 = Y * mis_pat
        cp_X = np.asfortranarray(X.T @ X)
        cp_X_rm = [np.asfortranarray(X[mis_pat[:, k] == 0].T @ X[mis_pat[:, k] == 0]) for k in range(q)]
        cp_Y_X = np.asfortranarray(Y0.T @ X)
        bx = cp_X.T @ m1 - np.stack([cp_X_rm[k].T @ m1[:, k] for k in range(q)], axis=1)
        out.update(cp_X=cp_X, cp_X_rm=cp_X_rm, cp_Y_X=cp_Y_X, cp_betaX_X=np.asfortranarray(bx),
                   sig2_beta_vb=np.asfortranarray(rng.uniform(0.005, 0.02, size=(p, q))))
    else:
        cp_X = np.asfortranarray(X.T @ X)
        out.update(cp_X=cp_X, cp_Y_X=np.asfortranarray(Y.T @ X), cp_betaX_X=np.asfortranarray(cp_X.T @ m1),
                   sig2_beta_vb=rng.uniform(0.005, 0.02, size=q))
    return out
