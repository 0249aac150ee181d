"""CPU: the kNN degradation probe without a device.

* tests/knn_restatement.py (the yardstick of tests/test_gpu_knn.py) and the product's ``train_test_indices`` / ``classification_report``
  against scikit-learn where it is installed: ``train_test_split``, ``KNeighborsClassifier(5)`` (``predict`` and ``kneighbors``) and
  ``classification_report(output_dict=True)`` on the three seeded cluster fixtures over the reference's five seeds -- indices, predictions,
  neighbour lists and their order all equal.
* the fixtures leave no query undecidable (tests/knn_restatement.py ``decidable``): asserted here and again on the GPU.
* the refusals of dcpt_pdist2_fwd / dcpt_knn_vote_fwd and the workspace query need no device.
* the ``--features`` flow of basicsr/knn.py on a saved directory, up to the "no CPU fallback" error."""
import os
import warnings

import numpy as np
import pytest
import torch

import knn_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def probes():
    """the restatement's whole probe per fixture: computed once, shared, never modified"""
    out = {}
    for name in R.FIXTURES:
        x, labels = R.clusters(name)
        out[name] = (x, labels, R.probe(x, labels))
    return out


@pytest.mark.parametrize("name", list(R.FIXTURES))
def test_restatement_and_product_against_scikit_learn(name, probes):
    pytest.importorskip("sklearn")
    from sklearn.metrics import classification_report as sk_report
    from sklearn.model_selection import train_test_split
    from sklearn.neighbors import KNeighborsClassifier

    from basicsr.utils import classification_report, train_test_indices

    x, labels, runs = probes[name]
    for run in runs:
        seed = run["seed"]
        idx_train, idx_test = train_test_split(np.arange(len(x)), test_size=0.33, random_state=seed)
        assert np.array_equal(run["train"], idx_train) and np.array_equal(run["test"], idx_test)
        tr, te = train_test_indices(len(x), 0.33, seed)
        assert np.array_equal(tr, idx_train) and np.array_equal(te, idx_test)
        clf = KNeighborsClassifier(n_neighbors=5).fit(x[idx_train], labels[idx_train])
        pred = clf.predict(x[idx_test])
        _, nbr = clf.kneighbors(x[idx_test])
        print(f"{name} seed {seed}: {int((pred != run['pred']).sum())} predictions and {int((nbr != run['nbr']).any(1).sum())} neighbour lists differ "
              f"from scikit-learn's; {run['ties']} vote ties, {run['undecidable']} undecidable queries of {len(idx_test)}")
        assert np.array_equal(pred, run["pred"]) and np.array_equal(nbr, run["nbr"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = sk_report(labels[idx_test], pred, output_dict=True, zero_division=0)
            want_text = sk_report(labels[idx_test], pred, zero_division=0)
        got, text = classification_report(labels[idx_test], pred)
        for rep in (got, run["report"]):
            assert list(rep) == list(want)
            for key, val in want.items():
                if key == "accuracy":
                    assert abs(rep[key] - val) <= 1e-15
                else:
                    assert rep[key]["support"] == val["support"]
                    assert all(abs(rep[key][m] - val[m]) <= 1e-15 for m in ("precision", "recall", "f1-score")), (key, rep[key], val)
        assert text == want_text


def test_report_with_a_label_that_is_never_predicted_or_never_true():
    """zero denominators give 0: label 3 is never predicted (precision), label 9 never true (recall)"""
    from basicsr.utils import classification_report

    rep, text = classification_report([1, 1, 3, 3, 2], [1, 2, 9, 1, 2])
    assert rep["3"] == {"precision": 0.0, "recall": 0.0, "f1-score": 0.0, "support": 2}
    assert rep["9"] == {"precision": 0.0, "recall": 0.0, "f1-score": 0.0, "support": 0}
    assert rep["accuracy"] == 0.4 and rep["macro avg"]["support"] == 5 and list(rep) == ["1", "2", "3", "9", "accuracy", "macro avg", "weighted avg"]
    assert rep == R.report([1, 1, 3, 3, 2], [1, 2, 9, 1, 2])
    assert text.splitlines()[0].split() == ["precision", "recall", "f1-score", "support"] and "weighted avg" in text.splitlines()[-1]
    with pytest.raises(ValueError):
        classification_report([1, 2], [1])


def test_split_rule():
    from basicsr.utils import train_test_indices

    tr, te = train_test_indices(500, 0.33, 223)
    assert len(te) == 165 and len(tr) == 335 and sorted(np.concatenate([tr, te]).tolist()) == list(range(500))
    assert len(train_test_indices(60, 0.33, 0)[1]) == 20 and len(train_test_indices(120, 0.33, 0)[1]) == 40   # ceil(19.8), ceil(39.6)
    with pytest.raises(ValueError):
        train_test_indices(1, 0.33, 0)
    with pytest.raises(ValueError):
        train_test_indices(10, 1.0, 0)


def test_fixtures_leave_no_query_undecidable(probes):
    for name, (_, _, runs) in probes.items():
        bad = [(r["seed"], r["undecidable"]) for r in runs if r["undecidable"]]
        assert not bad, f"{name}: undecidable queries {bad}; choose another fixture seed"
    xb = R.bf16_round(R.clusters("120x17")[0])
    assert not any(r["undecidable"] for r in R.probe(xb, R.clusters("120x17")[1]))


def test_restatement_vote_and_order_rules():
    d = np.array([[3.0, 1.0, np.nan, 1.0, np.inf, 0.0, -0.0]])
    assert R.neighbours(d[0], 7).tolist() == [5, 6, 1, 3, 0, 4, 2]          # stable: equal distances by position, -0 == +0, NaN last
    assert R.vote([7, -3, 7, -3, 100]) == -3 and R.vote([100]) == 100 and R.vote([2, 1, 1, 2, 3]) == 1
    assert R.bf16_round(np.array([1.00390625, 1.01171875, 3.0], np.float32)).tolist() == [1.0, 1.015625, 3.0]   # ties to even


def test_pdist2_refusals_and_workspace_query_need_no_device():
    from dcpt_amd import _lib

    lib = _lib.load()
    q = lib.dcpt_pdist2_ws_bytes
    assert q(17, 33, 130, 3) >= 8 * 3 * (17 * 33 + 17 + 33) and q(17, 33, 130, 3) > q(17, 33, 130, 1) > 0
    assert q(500, 500, 524288, 0) > 8 * 500 * 500                       # the library's own split
    assert q(1, 1, 1, 0) > 0 and q(1, 1, 1, 1) > 0 and q(1, 1, 5, 2) > 0
    for bad in ((0, 4, 4, 1), (4, 0, 4, 1), (4, 4, 0, 1), (65536, 4, 4, 1), (4, 65536, 4, 1), (4, 4, 8, -1), (4, 4, 8, 3), (4, 4, 9, 4)):
        assert q(*bad) == 0, bad
    assert q(65535, 1, 9, 3) > 0

    def call(xq=1, xt=1, d2=1, ws=1, nws=1 << 30, Nq=4, Nt=5, D=8, ldq=8, ldt=8, ldd=5, ksplit=1, flags=0):
        rc = lib.dcpt_pdist2_fwd(xq, xt, d2, ws, nws, Nq, Nt, D, ldq, ldt, ldd, ksplit, flags, None)
        return rc, lib.dcpt_last_error()

    for kw, word in ((dict(xq=None), b"null"), (dict(xt=None), b"null"), (dict(d2=None), b"null"), (dict(ws=None), b"null"),
                     (dict(Nq=0), b"at least 1"), (dict(Nt=0), b"at least 1"), (dict(D=0), b"at least 1"), (dict(Nq=65536), b"65535"),
                     (dict(Nt=65536, ldd=65536), b"65535"), (dict(ldq=7), b"leading dimension"), (dict(ldt=7), b"leading dimension"),
                     (dict(ldd=4), b"leading dimension"), (dict(ksplit=-1), b"ksplit"), (dict(ksplit=3), b"ksplit"), (dict(flags=2), b"flags"),
                     (dict(flags=-1), b"flags"), (dict(nws=q(4, 5, 8, 1) - 1), b"workspace too small")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg, (kw, rc, msg)


def test_knn_vote_refusals_need_no_device():
    from dcpt_amd import _lib

    lib = _lib.load()

    def call(d2=1, ldd=8, q=1, t=1, lab=1, S=2, nq=3, nt=6, k=5, nbr=1, nd=1, pred=1):
        rc = lib.dcpt_knn_vote_fwd(d2, ldd, q, t, lab, S, nq, nt, k, nbr, nd, pred, None)
        return rc, lib.dcpt_last_error()

    for kw, word in ((dict(d2=None), b"null"), (dict(q=None), b"null"), (dict(t=None), b"null"), (dict(lab=None), b"null"),
                     (dict(nbr=None), b"null"), (dict(nd=None), b"null"), (dict(pred=None), b"null"), (dict(S=0), b"at least 1"),
                     (dict(nq=0), b"at least 1"), (dict(nt=0, k=1), b"at least 1"), (dict(k=0), b"k must"), (dict(k=33, nt=100), b"k must"),
                     (dict(k=6, nt=5), b"k must")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg, (kw, rc, msg)


def test_python_ops_refuse_cpu_tensors_and_bad_arguments():
    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    with pytest.raises(_lib.DcptHipError, match="no CPU fallback"):
        DF.pairwise_sqdist(torch.zeros(4, 8))
    with pytest.raises(_lib.DcptHipError, match="no CPU fallback"):
        DF.knn_vote(torch.zeros(4, 4, dtype=torch.float64), [0, 1, 0, 1], [[0, 1, 2]], [[3]], 1)
    with pytest.raises(_lib.DcptHipError):
        DF.pairwise_sqdist(np.zeros((4, 8), np.float32))


def test_features_flow_of_the_command_reaches_the_no_cpu_fallback_error(tmp_path, monkeypatch):
    """``basicsr/knn.py --features DIR`` loads the reference's dump and runs the probe; without a device the distances raise (where a
    device is present the command is told there is none: tests/test_gpu_knn.py runs it to its end)"""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from basicsr.knn import knn_pipeline, load_features
    from dcpt_amd import _lib

    x, labels = R.clusters("60x1000")
    np.save(tmp_path / "lr_features_1.npy", x)
    np.save(tmp_path / "lr_features_2.npy", x[:, :64].reshape(60, 4, 4, 4))   # (a map that was not flattened)
    np.save(tmp_path / "lr_labels.npy", labels)
    feats, lab = load_features(str(tmp_path))
    assert [f.shape for f in feats] == [(60, 1000), (60, 64)] and np.array_equal(lab, labels)
    with pytest.raises(_lib.DcptHipError, match="no CPU fallback"):
        knn_pipeline(ROOT, ["--features", str(tmp_path), "--out", str(tmp_path / "out")])
    assert not (tmp_path / "out" / "knn_report.json").exists()
    with pytest.raises(SystemExit):
        knn_pipeline(ROOT, [])


def test_hook_rule_is_shared_with_the_pretraining_model():
    """DCPTModel.select_hook_modules and FeatureTaps pick with one function"""
    from basicsr.archs.nafnet_arch import NAFNetBaseline
    from basicsr.utils import FeatureTaps, select_hook_modules

    net = NAFNetBaseline(3, 8, 1, [1, 1], [1, 2])
    assert [n for n, _ in select_hook_modules(net, "decoder", 1)] == ["decoder0.0", "decoder1.0", "decoder1.1"]
    assert [n for n, _ in select_hook_modules(net, "decoder", 0)] == ["decoder0", "decoder1"]
    with pytest.raises(ValueError, match="hook_names is required"):
        select_hook_modules(net, None)
    with pytest.raises(ValueError, match="hook_depth"):
        select_hook_modules(net, "decoder", 2)
    with pytest.raises(ValueError, match="no module"):
        FeatureTaps(net, "nothing_like_this")
    taps = FeatureTaps(net, "decoder", 0, rows=2)
    assert [n for n, _ in taps.picked] == ["decoder0", "decoder1"]
    taps.close()
    assert not any(m._forward_hooks for m in net.modules())
