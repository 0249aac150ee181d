"""GPU: exact t-SNE on the device -- dcpt_tsne_affinity_fwd / dcpt_tsne_joint_fwd / dcpt_tsne_steps_fwd / dcpt_tsne_kl_fwd of
dcpt_amd/csrc/tsne.hip through dcpt_amd.functional, basicsr.utils.tsne_embed and the command basicsr/tsne.py -- against
tests/tsne_restatement.py, the float64 numpy restatement that tests/test_tsne_cpu.py ties to scikit-learn.  The distances of every case are
float32 values, so scikit-learn (which rounds them), the restatement and the kernels see the same numbers.

Bounds (u = 2^-53; none of them comes from what the kernels gave):
* beta and the step counts: bit for bit.  beta moves by doubling, halving and midpoints, exact dyadic arithmetic, so the sequences agree
  as long as every decision does; the restatement asserts that every visited | |e| - 1e-5 | exceeds 1e-9 (smallest of any case 2.2e-8;
  the rounding of e is below 1e-12).
* pcond and P: 64 N u of the row's largest entry -- two one-ulp exponentials and an N-term sum in another order cannot exceed that.
* one evaluation: a sum of n terms in any order errs by at most n u sum |terms|, and the kernels' longest chain is N / 64 + 6 additions for
  a row and N / 256 + 8 over the rows, below N + 16; a term (P' - Q) w (y_i - y_j) carries a few roundings of its own and, through
  Q = w / Z, the N u of Z, which moves it by |Q w (y_i - y_j)| N u.  So |g - g_ref| <= E_g = 2 (N + 16) u g_abs with
  g_abs = 4 sum_j (|(P' - Q) w dy| + |Q w dy|), twice because both sides err; likewise |kl - kl_ref| <= 2 (N + 16) u (sum |terms| +
  sum |P'|) (a relative error r of Q moves a term by |P'| r).  gains are bit for bit (the first step multiplies by 0.8; for a moving
  state the restatement asserts that no |update g| lies within 1e-12 of the largest, so every branch is decided); update errs by
  lr gains E_g + 4 u (|momentum update| + |lr g gains|), Y by that + 2 u |y|, the gradient norm by |gains E_g|_2 + (N + 16) u |g gains|_2.
* ten steps: 1000 times the difference between the restatement and scikit-learn's float64 descent on the same case (TEN_STEP_CPU_DIFF,
  printed by tools/make_golden_tsne.py); longer trajectories amplify rounding to order 1 and are not compared.
Every bounded case prints its figure before it asserts."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import tsne_restatement as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
# tools/make_golden_tsne.py: ten steps, restatement vs scikit-learn's _gradient_descent, relative to the largest coordinate
TEN_STEP_CPU_DIFF = {"n37": 5.911e-14, "n150": 3.024e-14}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dcpt_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case(name):
    """the restatement of a case, computed once and shared (read-only)"""
    d2, perplexity = R.case_d2(name)
    pcond, beta, steps, margin = R.cond_affinities(d2, perplexity)
    out = dict(d2=d2, perplexity=perplexity, pcond=pcond, beta=beta, steps=steps, margin=margin, P=R.joint(pcond))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _bits(t):
    return t.contiguous().view(torch.int64)


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---- affinities ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pad", [(n, 0) for n in R.AFFINITY_CASES] + [("n65", 3)])
def test_affinities_equal_the_restatement(name, pad, dev):
    """N = 2, 3, 37, 63, 64, 65, 150, 257, 1030, duplicate rows, distances above 1e5 (s == 0 at beta = 1) and a padded leading dimension
    whose gap and whose diagonal hold NaNs (neither is read)"""
    from dcpt_amd import functional as DF

    c = _case(name)
    N = len(c["d2"])
    assert c["margin"] > R.MARGIN, f"a visited |e| lies within {c['margin']:.2e} of the tolerance: the step counts are not comparable"
    buf = torch.full((N, N + pad), float("nan"), dtype=torch.float64, device=dev)
    buf[:, :N] = _dev(c["d2"], dev)
    d2, idx = buf[:, :N], torch.arange(N, device=dev)
    d2[idx, idx] = float("nan")
    P, beta, steps, pcond = DF.tsne_affinities(d2, c["perplexity"], return_conditional=True)
    P2, beta2, steps2 = DF.tsne_affinities(d2, c["perplexity"])   # (P written over the conditional affinities)
    assert torch.equal(_bits(P), _bits(P2)) and torch.equal(_bits(beta), _bits(beta2)) and torch.equal(steps, steps2)
    assert torch.equal(_bits(P), _bits(P.t())) and (P.diagonal() == 0).all() and (pcond.diagonal() == 0).all()
    assert np.array_equal(steps.cpu().numpy(), c["steps"]), (steps.cpu().numpy() - c["steps"]).nonzero()
    assert np.array_equal(beta.cpu().numpy().view(np.int64), c["beta"].view(np.int64))
    tol = 64 * N * U
    for what, got, want in (("pcond", pcond.cpu().numpy(), c["pcond"]), ("P", P.cpu().numpy(), c["P"])):
        ratio = float((np.abs(got - want) / (tol * want.max(axis=1, keepdims=True))).max())
        print(f"{name} pad {pad} {what}: worst |got - want| / (64 N u rowmax) = {ratio:.4f} (N = {N}, margin {c['margin']:.2e}, steps "
              f"{c['steps'].min()}..{c['steps'].max()})")
        assert np.isfinite(got).all() and ratio <= 1.0


# ---- one evaluation and one step -------------------------------------------------------------------------------------------------------------
def _bounds(P, Y, update, gains, ex, mom, lr):
    N = len(P)
    kl, g, kl_abs, g_abs = R.kl_grad(P, Y, ex)
    Y1, u1, gn1, kl_, gnorm, _ = R.step(P, Y, update, gains, ex, mom, lr)
    E_g = 2 * (N + 16) * U * g_abs
    E_kl = 2 * (N + 16) * U * kl_abs
    E_u = lr * gn1 * E_g + 4 * U * (np.abs(mom * update) + np.abs(lr * g * gn1))
    E_y = E_u + 2 * U * np.abs(Y1)
    E_n = np.sqrt(((gn1 * E_g) ** 2).sum()) + (N + 16) * U * gnorm
    return dict(kl=kl, g=g, Y=Y1, update=u1, gains=gn1, gnorm=gnorm, E_g=E_g, E_kl=E_kl, E_u=E_u, E_y=E_y, E_n=E_n)


def _check_step(what, dev, P, Y, update, gains, ex, mom, lr):
    from dcpt_amd import functional as DF

    b = _bounds(P, Y, update, gains, ex, mom, lr)
    Pd, Yd, ud, gd = (_dev(a, dev) for a in (P, Y, update, gains))
    kl, grad = DF.tsne_kl(Pd, Yd, ex)
    assert torch.equal(_bits(Yd), _bits(_dev(Y, dev)))   # (the evaluation moves nothing)
    stats = DF.tsne_steps(Pd, Yd, ud, gd, 1, ex, mom, lr)
    kl, grad, stats, Yg, ug, gg = (t.cpu().numpy() for t in (kl, grad, stats, Yd, ud, gd))
    figs = {"grad": (np.abs(grad - b["g"]) / b["E_g"]).max(), "kl": abs(kl - b["kl"]) / b["E_kl"], "stats kl": abs(stats[0] - b["kl"]) / b["E_kl"],
            "update": (np.abs(ug - b["update"]) / b["E_u"]).max(), "Y": (np.abs(Yg - b["Y"]) / b["E_y"]).max(),
            "grad norm": abs(stats[1] - b["gnorm"]) / b["E_n"]}
    print(f"{what}: kl {b['kl']:.6e}, |g| {b['gnorm']:.3e}; worst error / bound: " + ", ".join(f"{k} {v:.4f}" for k, v in figs.items()))
    assert np.array_equal(gg.view(np.int64), b["gains"].view(np.int64)), "gains"
    assert all(np.isfinite(v) and v <= 1.0 for v in figs.values())


@pytest.mark.parametrize("scale", [1.0, 1e-4, 1e3])
@pytest.mark.parametrize("ex", [12.0, 1.0])
@pytest.mark.parametrize("name", ["n2", "n65", "n257", "n1030"])
def test_one_step_within_the_derived_bounds(name, ex, scale, dev):
    """from the state a phase starts with (update 0, gains 1) at the "random" rule's draw scaled by 1, 1e-4 (the rule itself: w near 1) and
    1e3 (w near 1e-6); two workgroups and more, rows past the last workgroup's four"""
    P = _case(name)["P"]
    N = len(P)
    Y = R.case_y(N, 11, scale)
    _check_step(f"{name} ex {ex} scale {scale}", dev, P, Y, np.zeros_like(Y), np.ones_like(Y), ex, 0.5, max(N / 12.0 / 4.0, 50.0))


@pytest.mark.parametrize("name", ["n65", "n257"])
def test_second_step_takes_both_gain_branches(name, dev):
    """the second step of a two-step case: the state after the restatement's first step (update nonzero) goes to the device, so the gain
    rule meets both signs; no |update g| of the restatement lies within 1e-12 of the largest, so every branch is decided"""
    P = _case(name)["P"]
    N = len(P)
    Y0 = R.case_y(N, 11, 1.0)
    lr = 50.0
    Y1, u1, g1, _, _, _ = R.step(P, Y0, np.zeros_like(Y0), np.ones_like(Y0), 12.0, 0.5, lr)
    Y1 = Y1 + 0.5 * R.case_y(N, 12, 1.0)   # (moved off the descent direction, or every product update g would keep one sign)
    prod = u1 * R.kl_grad(P, Y1, 12.0)[1]
    assert np.abs(prod).min() > 1e-12 * np.abs(prod).max()
    assert (prod < 0).any() and (prod > 0).any()
    _check_step(f"{name} second step", dev, P, Y1, u1, g1, 12.0, 0.5, lr)


@pytest.mark.parametrize("name", R.TEN_STEP_CASES)
def test_ten_steps(name, dev):
    from dcpt_amd import functional as DF

    P = _case(name)["P"]
    Y0 = R.random_init(len(P), 3)
    want, wu, wg, wkl, wgn = R.steps(P, Y0, np.zeros_like(Y0), np.ones_like(Y0), 10, *R.TEN_STEP_PARAMS)
    Yd = _dev(Y0, dev)
    ud, gd = torch.zeros_like(Yd), torch.ones_like(Yd)
    stats = DF.tsne_steps(_dev(P, dev), Yd, ud, gd, 10, *R.TEN_STEP_PARAMS).cpu().numpy()
    tol = 1000 * TEN_STEP_CPU_DIFF[name]
    err = np.abs(Yd.cpu().numpy() - want).max() / np.abs(want).max()
    print(f"{name}: ten steps, max |Y - Y_ref| / max |Y_ref| = {err:.3e} (tolerance {tol:.3e}); kl {stats[0]:.12e} vs {wkl:.12e}, "
          f"|g| {stats[1]:.6e} vs {wgn:.6e}")
    assert err <= tol
    assert np.array_equal(gd.cpu().numpy().view(np.int64), wg.view(np.int64))
    assert abs(stats[0] - wkl) <= tol * abs(wkl) and abs(stats[1] - wgn) <= tol * wgn


def test_chunks_give_the_same_bits_and_the_statistics_are_those_before_the_last_move(dev):
    """50 steps in one call and in 5 calls of 10: Y, update, gains and the statistics bit for bit (an odd and an even number of steps end
    in different halves of the ping-pong: 7 + 43 as well); the statistics of a call are the KL at the Y before its last move"""
    from dcpt_amd import functional as DF

    P = _case("n257")["P"]
    N = len(P)
    Pd = _dev(P, dev)

    def run(chunks):
        Y = _dev(R.random_init(N, 5), dev)
        u, g, stats = torch.zeros_like(Y), torch.ones_like(Y), None
        for n in chunks:
            stats = DF.tsne_steps(Pd, Y, u, g, n, 12.0, 0.5, 50.0)
        return Y, u, g, stats

    a = run([50])
    for chunks in ([10] * 5, [7, 43], [49, 1]):
        b = run(chunks)
        assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b)), chunks
    Y, u, g, _ = run([49])
    kl, _ = DF.tsne_kl(Pd, Y, 12.0)
    Y49 = Y.cpu().numpy()
    stats = DF.tsne_steps(Pd, Y, u, g, 1, 12.0, 0.5, 50.0)
    assert torch.equal(_bits(stats), _bits(a[3])) and torch.equal(_bits(Y), _bits(a[0]))
    ref, _, kl_abs, _ = R.kl_grad(P, Y49, 12.0)
    E = 2 * (N + 16) * U * kl_abs
    print(f"kl of the last call {float(stats[0]):.15e}, tsne_kl at the Y before its last move {float(kl):.15e}, restatement {ref:.15e}, "
          f"bound {E:.3e}")
    assert abs(float(stats[0]) - float(kl)) <= E and abs(float(kl) - ref) <= E
    nothing = DF.tsne_steps(Pd, Y, u, g, 0, 12.0, 0.5, 50.0)   # n_steps = 0 touches nothing
    assert torch.equal(_bits(Y), _bits(a[0])) and torch.isnan(nothing).all()


# ---- the driver and the command ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("init", ["pca", "random"])
def test_driver_separates_the_blobs(init, dev):
    """150 points, five separated blobs in 50 dimensions, max_iter 500: every point's 5 nearest embedding neighbours carry its label --
    scikit-learn's exact method and the restatement's schedule give 1.0 on this data for both starts (tests/test_tsne_cpu.py shows it
    for this seed) --, the reported KL is the restatement's KL of the returned embedding at 1e-10 and lies below that of the start, the
    history has one entry per 50 iterations, and a second run returns the same bits"""
    from basicsr.utils import neighbour_label_share, pca_init_from_sqdist, tsne_embed
    from dcpt_amd import functional as DF

    X, labels, _ = R.driver_data()
    x = torch.from_numpy(X).to(dev)
    res = tsne_embed(x, max_iter=500, init=init)
    Y = res["embedding"]
    assert Y.shape == (150, 2) and Y.dtype == np.float64 and np.isfinite(Y).all()
    share = neighbour_label_share(Y, labels, 5)
    # the restatement's affinities of the distances the device computed from the unit-length rows
    d2 = DF.pairwise_sqdist(x / x.norm(dim=1, keepdim=True)).cpu().numpy()
    P = R.joint(R.cond_affinities(d2, 30.0)[0])
    kl = R.kl_grad(P, Y)[0]
    Y0 = pca_init_from_sqdist(d2) if init == "pca" else R.random_init(150, 0)
    kl0 = R.kl_grad(P, Y0)[0]
    print(f"init {init}: share {share}, reported kl {res['kl_divergence']:.12f}, restatement at the returned Y {kl:.12f}, at the start "
          f"{kl0:.6f}, n_iter {res['n_iter']}, history {[(h[0], round(h[1], 4)) for h in res['history']]}")
    assert share == 1.0 and R.neighbour_purity(Y, labels) == 1.0
    assert abs(res["kl_divergence"] - kl) <= 1e-10
    assert res["kl_divergence"] < kl0
    assert res["n_iter"] == 499 and [h[0] for h in res["history"]] == list(range(49, 500, 50))
    again = tsne_embed(x, max_iter=500, init=init)
    assert np.array_equal(again["embedding"].view(np.int64), Y.view(np.int64)) and again["history"] == res["history"]
    given = tsne_embed(x, max_iter=500, init=Y0)   # an (N, 2) array is taken as given
    assert np.array_equal(given["embedding"].view(np.int64), Y.view(np.int64))


def test_the_command_on_the_shipped_option(tmp_path, dev):
    """basicsr/tsne.py on options/knn/knn_NAFNet_5d.yml with its synthetic sets (12 images of 32 x 32 each, the three decoder groups):
    tsne_<level>.npy and tsne.json; then --features on a dump of the same shape"""
    from basicsr.tsne import tsne_pipeline

    force = [f"datasets:test_{i}:{k}={v}" for i in range(1, 6) for k, v in (("max_per_set", 12), ("size", 32))]
    rep = tsne_pipeline(ROOT, ["-opt", os.path.join(ROOT, "options", "knn", "knn_NAFNet_5d.yml"), "--out", str(tmp_path), "--max_iter", "500",
                               "--force_yml", *force, "knn:hook_depth=0", "knn:batch_size=16"])
    assert rep == json.load(open(tmp_path / "tsne.json"))
    assert rep["n"] == 60 and rep["labels"] == [1, 2, 3, 4, 5] and [lv["module"] for lv in rep["levels"]] == ["decoder0", "decoder1", "decoder2"]
    for lv in rep["levels"]:
        Y = np.load(tmp_path / f"tsne_{lv['level']}.npy")
        assert Y.shape == (60, 2) and Y.dtype == np.float64 and np.isfinite(Y).all()
        assert np.isfinite(lv["kl_divergence"]) and lv["n_iter"] <= 499 and 0.0 <= lv["neighbour_label_share"] <= 1.0
        assert lv["picture"] == os.path.isfile(tmp_path / f"tsne_{lv['level']}.png")
    dump = tmp_path / "dump"
    os.makedirs(dump)
    X, labels, _ = R.driver_data()
    np.save(dump / "lr_features_1.npy", X)
    np.save(dump / "lr_labels.npy", labels + 1)
    rep = tsne_pipeline(ROOT, ["--features", str(dump), "--out", str(tmp_path / "o2"), "--max_iter", "500"])
    assert rep["levels"][0]["neighbour_label_share"] == 1.0 and np.load(tmp_path / "o2" / "tsne_1.npy").shape == (150, 2)
