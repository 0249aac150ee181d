"""CPU: the float64 restatement of exact t-SNE (tests/tsne_restatement.py) against scikit-learn -- recorded in tests/golden/tsne.npz by
tools/make_golden_tsne.py, and directly where scikit-learn is installed --, the PCA start against scikit-learn's PCA, and what the t-SNE
entry points, ops, driver and command do without a device: the workspace query, every refusal, option parsing, the no-CPU-path error."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tsne_restatement as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "tsne.npz")
# the restatement and scikit-learn differ by sums of N <= 150 terms in another order and one-ulp functions: observed 0 .. 9e-16 for P
# relative to its largest entry and 1e-15 for KL and gradient; the bounds leave two orders
P_TOL, KG_TOL = 1e-13, 1e-12


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name in R.GOLDEN_CASES:
        d2, perplexity = R.case_d2(name)
        pcond, beta, steps, margin = R.cond_affinities(d2, perplexity)
        out[name] = dict(d2=d2, perplexity=perplexity, pcond=pcond, beta=beta, steps=steps, margin=margin, P=R.joint(pcond))
    return out


def _check_p(P, want):
    assert np.abs(P - want).max() <= P_TOL * want.max()
    assert (P == P.T).all() and (np.diag(P) == 0).all()


@pytest.mark.parametrize("name", R.GOLDEN_CASES)
def test_restatement_equals_the_recorded_scikit_learn(cases, name):
    g, c = np.load(GOLDEN), cases[name]
    _check_p(c["P"], g[f"P_{name}"])
    N = len(c["P"])
    kl, grad, _, _ = R.kl_grad(c["P"], R.case_y(N, 7, 1.0))
    assert abs(kl - g[f"kl_{name}"]) <= KG_TOL * abs(g[f"kl_{name}"])
    assert np.abs(grad - g[f"grad_{name}"]).max() <= KG_TOL * np.abs(g[f"grad_{name}"]).max()
    assert c["margin"] > R.MARGIN   # (the GPU test compares step counts: no visited |e| may lie at the tolerance)


def test_the_three_edge_conditions_occur(cases):
    """what the GPU test relies on, shown here first: N = 2 can never reach its entropy and runs all 100 steps (beta = 2^-100); duplicate
    rows give zero off-diagonal distances; at distances above 1e5 every exponential is 0 at beta = 1 and the sum takes the 1e-8 branch --
    and in all three the restatement equals scikit-learn's function (the test above)"""
    assert (cases["n2"]["steps"] == 99).all() and (cases["n2"]["beta"] == 2.0 ** -100).all()
    d = cases["dup"]["d2"]
    assert (d[0, 3], d[1, 4], d[2, 5]) == (0.0, 0.0, 0.0)
    off = ~np.eye(len(cases["far"]["d2"]), dtype=bool)
    assert np.exp(-cases["far"]["d2"][off]).max() == 0.0 and cases["far"]["steps"].min() > 10


def test_ten_steps_against_the_recording():
    """the restatement's descent and scikit-learn's _gradient_descent (float64) after ten iterations: 5.9e-14 and 3.0e-14 of the largest
    coordinate when recorded; 1e-12 here.  Longer trajectories are not comparable (5e-9 after 25 iterations, order 1 after 60)."""
    g = np.load(GOLDEN)
    for name in R.TEN_STEP_CASES:
        d2, perplexity = R.case_d2(name)
        P = R.joint(R.cond_affinities(d2, perplexity)[0])
        Y0 = R.random_init(len(P), 3)
        Y = R.steps(P, Y0, np.zeros_like(Y0), np.ones_like(Y0), 10, *R.TEN_STEP_PARAMS)[0]
        want = g[f"y10_{name}"]
        assert np.abs(Y - want).max() <= 1e-12 * np.abs(want).max()


def test_restatement_equals_scikit_learn_directly(cases):
    T = pytest.importorskip("sklearn.manifold._t_sne")
    from scipy.spatial.distance import squareform

    for name, c in cases.items():
        Pc = T._joint_probabilities(c["d2"].astype(np.float32), c["perplexity"], 0)
        _check_p(c["P"], squareform(Pc))
        N = len(c["P"])
        for scale in (1e-4, 1.0, 1e3):
            Y = R.case_y(N, 7, scale)
            kl, grad = T._kl_divergence(Y.ravel().copy(), Pc, 1.0, N, 2)
            got_kl, got_grad, _, _ = R.kl_grad(c["P"], Y)
            assert abs(got_kl - kl) <= KG_TOL * abs(kl)
            assert np.abs(got_grad - grad.reshape(N, 2)).max() <= KG_TOL * np.abs(grad).max()


def test_pca_start_equals_scikit_learn_pca():
    """the classical-MDS start from the distances alone against PCA(n_components=2, svd_solver="full") of the rows, up to the sign of a
    column, at 1e-8 relative; the product's function and the restatement's"""
    dec = pytest.importorskip("sklearn.decomposition")
    from basicsr.utils.tsne import pca_init_from_sqdist

    X = R.driver_data()[0].astype(np.float64)
    d2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    want = dec.PCA(n_components=2, svd_solver="full").fit_transform(X)
    want = want / np.std(want[:, 0]) * 1e-4
    for fn in (pca_init_from_sqdist, R.pca_init):
        Y = fn(d2)
        assert abs(np.std(Y[:, 0]) - 1e-4) <= 1e-18
        for c in range(2):
            assert Y[np.argmax(np.abs(Y[:, c])), c] > 0
            err = min(np.abs(Y[:, c] - want[:, c]).max(), np.abs(Y[:, c] + want[:, c]).max())
            assert err <= 1e-8 * np.abs(want[:, c]).max()


def test_schedule_separates_the_blobs_as_scikit_learn_does():
    """the driver test's data (150 points, five separated blobs in 50 dimensions, unit-length rows, max_iter 500): under the restatement's schedule every
    point's 5 nearest embedding neighbours carry its label for both starts, the KL falls, and the history has one entry per 50
    iterations; scikit-learn's exact method gives the same share (1.0) where it is installed"""
    X, labels, d2 = R.driver_data()
    P = R.joint(R.cond_affinities(d2, 30.0)[0])
    for Y0 in (R.pca_init(d2), R.random_init(150, 0)):
        Y, kl, it, hist = R.schedule(P, Y0, max_iter=500)
        assert R.neighbour_purity(Y, labels) == 1.0
        assert it == 499 and [h[0] for h in hist] == list(range(49, 500, 50))
        assert kl < R.kl_grad(P, Y0)[0] and abs(kl - R.kl_grad(P, Y)[0]) < 0.05 * kl
    man = pytest.importorskip("sklearn.manifold")
    Ys = man.TSNE(n_components=2, method="exact", max_iter=500, init="random", random_state=0).fit_transform(X / np.linalg.norm(X, axis=1, keepdims=True))
    assert R.neighbour_purity(Ys.astype(np.float64), labels) == 1.0


# ---- the library, the ops and the command without a device ------------------------------------------------------------------------------
def test_workspace_query_needs_no_device():
    from dcpt_amd import _lib

    lib = _lib.load()
    q = lib.dcpt_tsne_steps_ws_bytes
    assert q(1) == 0 and q(0) == 0 and q(-3) == 0 and q(65536) == 0
    assert q(2) >= 2 * 2 * 8 + 3 * 2 * 8 and q(2) % 256 == 0
    assert q(65535) >= 5 * 65535 * 8 and q(4096) > q(500) > q(2)


def test_every_refusal_comes_before_any_launch():
    from dcpt_amd import _lib

    lib = _lib.load()
    p, big = 4096, 1 << 30   # a non-null, 16-byte aligned address that is never dereferenced, and a workspace size that is large enough

    def refused(rc, word):
        assert rc != 0 and word in lib.dcpt_last_error(), lib.dcpt_last_error()

    aff = lib.dcpt_tsne_affinity_fwd
    for args in ((None, 10, p, 10, p, p), (p, 10, None, 10, p, p), (p, 10, p, 10, None, p), (p, 10, p, 10, p, None)):
        refused(aff(*args, 10, 3.0, None), b"null")
    refused(aff(p, 10, p + 8192, 10, p, p, 1, 1.0, None), b"N must lie in 2 .. 65535")
    refused(aff(p, 70000, p + 8192, 70000, p, p, 65536, 30.0, None), b"N must lie in 2 .. 65535")
    for perp in (0.5, 10.0, 11.0, float("nan"), float("inf")):
        refused(aff(p, 10, p + 8192, 10, p, p, 10, perp, None), b"perplexity")
    refused(aff(p, 9, p + 8192, 10, p, p, 10, 3.0, None), b"leading dimension")
    refused(aff(p, 10, p + 8192, 9, p, p, 10, 3.0, None), b"leading dimension")
    refused(aff(p, 10, p, 10, p, p, 10, 3.0, None), b"pcond must not be d2")

    jnt = lib.dcpt_tsne_joint_fwd
    refused(jnt(None, 10, p, 10, p, big, 10, None), b"null")
    refused(jnt(p, 10, None, 10, p, big, 10, None), b"null")
    refused(jnt(p, 10, p, 10, p, big, 1, None), b"N must lie")
    refused(jnt(p, 9, p, 9, p, big, 10, None), b"leading dimension")
    refused(jnt(p, 10, p, 12, p, big, 10, None), b"same leading dimension")
    refused(jnt(p, 10, p, 10, None, big, 10, None), b"workspace too small")
    refused(jnt(p, 10, p, 10, p, lib.dcpt_tsne_steps_ws_bytes(10) - 1, 10, None), b"workspace too small")

    stp = lib.dcpt_tsne_steps_fwd
    ok = dict(P=p, ldp=10, Y=p, update=p, gains=p, stats=p, ws=p, ws_bytes=big, N=10, out_dims=2, n_steps=1, exaggeration=12.0, momentum=0.5,
              lr=50.0, min_gain=0.01)

    def steps_with(**kw):
        return stp(*{**ok, **kw}.values(), None)

    for k in ("P", "Y", "update", "gains", "stats"):
        refused(steps_with(**{k: None}), b"null")
    refused(steps_with(out_dims=3), b"only two output dimensions")
    refused(steps_with(N=1), b"N must lie")
    refused(steps_with(N=65536, ldp=65536), b"N must lie")
    refused(steps_with(ldp=9), b"leading dimension")
    refused(steps_with(n_steps=-1), b"n_steps")
    for k in ("exaggeration", "momentum", "lr", "min_gain"):
        refused(steps_with(**{k: float("nan")}), b"finite")
    refused(steps_with(Y=p + 8), b"16-byte aligned")
    refused(steps_with(ws=None), b"workspace too small")
    refused(steps_with(ws_bytes=lib.dcpt_tsne_steps_ws_bytes(10) - 1), b"workspace too small")

    kl = lib.dcpt_tsne_kl_fwd
    for args in ((None, 10, p, p, p), (p, 10, None, p, p), (p, 10, p, None, p), (p, 10, p, p, None)):
        refused(kl(*args, p, big, 10, 2, 1.0, None), b"null")
    refused(kl(p, 10, p, p, p, p, big, 10, 3, 1.0, None), b"only two output dimensions")
    refused(kl(p, 10, p, p, p, p, big, 1, 2, 1.0, None), b"N must lie")
    refused(kl(p, 9, p, p, p, p, big, 10, 2, 1.0, None), b"leading dimension")
    refused(kl(p, 10, p, p, p, p, big, 10, 2, float("inf"), None), b"finite")
    refused(kl(p, 10, p, p, p, p, 16, 10, 2, 1.0, None), b"workspace too small")


def test_host_tensors_raise_the_no_cpu_path_error():
    from basicsr.utils import tsne_embed
    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    P = torch.zeros(4, 4, dtype=torch.float64)
    Y = torch.zeros(4, 2, dtype=torch.float64)
    for call in (lambda: DF.tsne_affinities(P, 2.0), lambda: DF.tsne_steps(P, Y, Y.clone(), Y.clone(), 1, 12.0, 0.5, 50.0),
                 lambda: DF.tsne_kl(P, Y), lambda: DF.tsne_affinities(P.numpy(), 2.0), lambda: tsne_embed(torch.zeros(4, 8)),
                 lambda: tsne_embed(d2=P), lambda: tsne_embed(torch.zeros(4, 8), normalize=False)):
        with pytest.raises(_lib.DcptHipError):
            call()
    with pytest.raises(ValueError):
        tsne_embed()
    with pytest.raises(ValueError):
        tsne_embed(torch.zeros(4, 8), max_iter=100)


def test_command_line_and_option_block(tmp_path):
    from basicsr.tsne import EMBED_KEYS, embed_kwargs, label_names, parse_args, scatter_png
    from basicsr.utils.options import yaml_load

    a = parse_args(["-opt", "x.yml", "--out", "o", "--max_iter", "500", "--perplexity", "12.5"])
    assert (a.opt, a.features, a.out, a.max_iter, a.perplexity) == ("x.yml", None, "o", 500, 12.5)
    assert parse_args(["--features", "d"]).features == "d"
    for bad in ([], ["-opt", "x.yml", "--features", "d"]):
        with pytest.raises(SystemExit):
            parse_args(bad)
    # the shipped option files carry no tsne block: the defaults apply
    opt = yaml_load(os.path.join(ROOT, "options", "knn", "knn_NAFNet_5d.yml"))
    assert "tsne" not in opt and embed_kwargs(opt.get("tsne")) == {}
    assert label_names(None) == {1: "haze", 2: "motion-blur", 3: "noise", 4: "rain", 5: "low_light"}
    block = {"perplexity": 10, "max_iter": 500, "init": "random", "label_names": {3: "denoise", "6": "snow"}}
    assert embed_kwargs(block) == {"perplexity": 10, "max_iter": 500, "init": "random"} and set(embed_kwargs(block)) <= set(EMBED_KEYS)
    assert label_names(block)[3] == "denoise" and label_names(block)[6] == "snow" and label_names(block)[1] == "haze"
    with pytest.raises(ValueError):
        embed_kwargs({"n_iter": 2000})
    # every key of the block is an argument of the driver
    import inspect

    from basicsr.utils import tsne_embed
    assert set(EMBED_KEYS) <= set(inspect.signature(tsne_embed).parameters)
    # the picture is optional: with matplotlib a file, without it False and nothing else
    Y, labels = np.random.RandomState(0).standard_normal((10, 2)), np.arange(10) % 2 + 1
    made = scatter_png(str(tmp_path / "p.png"), Y, labels, label_names(None))
    assert made == os.path.isfile(tmp_path / "p.png")
