"""GPU: the kNN degradation probe -- dcpt_pdist2_fwd / dcpt_knn_vote_fwd of dcpt_amd/csrc/knn.hip through dcpt_amd.functional, basicsr.utils
(knn_probe, FeatureTaps) and the command basicsr/knn.py -- against tests/knn_restatement.py, the kernel-blind numpy restatement.

Bounds:
* distances: ``|d2 - T| <= E = 4 D 2^-53 (|q_i|^2 + |t_j|^2)`` with T the restatement's longdouble value.  Derived, not measured: products
  of fp32 / bf16 values are exact in fp64; an fp64 sum of D terms in any order errs by at most D 2^-53 sum |terms|; sum |q_k t_k| <=
  (n + m) / 2; three such sums and three final roundings give (2 D + 3) 2^-53 (n + m) <= E.  No element is excluded; the inputs have mean 3
  and spread 0.1, so n + m is about 1000 times a typical distance and the cancellation is exercised.
* integers in -8..8 at (20, 37, 256): every sum is exact in fp64, so d2 equals the integer result bit for bit -- the case that catches
  the f32 C/D map on the f64 MFMA (three of four results in the wrong row).
* at a fixed ksplit an entry depends on its two rows alone: permuted rows, duplicated rows, a sub-block, other leading dimensions and a
  second run give the same bits.
* the vote is bit for bit the restatement's on hand-made matrices (equal distances, vote ties, NaN / inf / -0, labels -3 / 7 / 100).
* end to end a query is decidable when every adjacent gap among its first k + 1 restated distances exceeds 2 max E of its row; undecidable
  queries may be left out, at most 0.1 % of a case, and the fixtures leave out NONE (asserted here and in tests/test_knn_cpu.py).

Every bounded case prints its figure before it asserts."""
import json
import os

import numpy as np
import pytest
import torch

import knn_restatement as R
from dcpt_amd.keyed_init import keyed_input

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dcpt_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int64)


def _strided(x, pad, dev):
    """the rows of x on the device with a row stride of D + pad (the gap holds NaNs: a kernel that read it would show)"""
    buf = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), dtype=x.dtype, device=dev)
    buf[:, :x.shape[1]] = x.to(dev)
    return buf[:, :x.shape[1]]


def _check(d2, xq, xt, what):
    """the derived bound, every element; prints the worst ratio first"""
    T, E = R.sqdist(xq, xt), R.error_bound(xq, xt)
    got = d2.cpu().numpy()
    err = np.abs(got.astype(np.longdouble) - T).astype(np.float64)
    worst = float((err / E).max())
    print(f"{what}: max |d2 - T| {float(err.max()):.3e}, worst |d2 - T| / E = {worst:.4f} over {err.size} entries (min T {float(T.min()):.3e}, "
          f"max n + m {float(E.max() / (4.0 * xq.shape[1] * 2.0 ** -53)):.3e})")
    assert np.isfinite(got).all() and (got >= 0).all() and worst <= 1.0


SHAPES = [(1, 1, 1, 0), (3, 5, 7, 0), (16, 16, 4, 0), (17, 33, 130, 0), (17, 33, 130, 1), (17, 33, 130, 3), (5, 200, 4099, 7)]


@pytest.mark.parametrize("Nq,Nt,D,ksplit", SHAPES)
def test_distances_within_the_derived_bound(Nq, Nt, D, ksplit, dev):
    """plain, with row strides above D, as bf16 and with xq is xt; output and workspace inside red-zone guards"""
    from kernel_trace import kernel_trace
    from redzone import redzone

    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    lib = _lib.load()
    tag = f"gpuknn.{Nq}x{Nt}x{D}"
    xq, xt = keyed_input(tag + ".q", (Nq, D), lo=2.9, hi=3.1), keyed_input(tag + ".t", (Nt, D), lo=2.9, hi=3.1)
    what = f"pdist2 ({Nq}, {Nt}, {D}) ksplit {ksplit}"
    with redzone() as rz:
        # the entry point itself on an output and a workspace of exactly the size they need
        nws = lib.dcpt_pdist2_ws_bytes(Nq, Nt, D, ksplit)
        assert nws > 0
        out = DF._workspace(dev, 8 * Nq * Nt)
        ws = DF._workspace(dev, nws)
        with kernel_trace() as t:
            DF._call(lib.dcpt_pdist2_fwd, (xq.to(dev), xt.to(dev), out, ws, nws), (Nq, Nt, D, D, D, Nt, ksplit, 0), dev)
        assert t.counts == {"knn.pdist2_norm": 1, "knn.pdist2_gemm": 1, "knn.pdist2_finish": 1}, t.counts
        plain = out.view(torch.float64).reshape(Nq, Nt).clone()
        _check(plain, xq.numpy(), xt.numpy(), what)
        # the Python op: the same bits; its workspace comes from the same allocator
        d2 = DF.pairwise_sqdist(xq.to(dev), xt.to(dev), ksplit=ksplit)
        assert d2.dtype == torch.float64 and tuple(d2.shape) == (Nq, Nt) and torch.equal(_bits(d2), _bits(plain))
        # row strides above D (odd: the rows lose their 16-byte alignment), the output rows too: the same bits
        wide = torch.full((Nq, Nt + 3), -1.0, dtype=torch.float64, device=dev)
        got = DF.pairwise_sqdist(_strided(xq, 5, dev), _strided(xt, 9, dev), ksplit=ksplit, out=wide[:, :Nt])
        assert got.data_ptr() == wide.data_ptr() and torch.equal(_bits(wide[:, :Nt]), _bits(plain)) and bool((wide[:, Nt:] == -1.0).all())
        # bf16 rows
        bq, bt = xq.to(torch.bfloat16), xt.to(torch.bfloat16)
        db = DF.pairwise_sqdist(bq.to(dev), bt.to(dev), ksplit=ksplit)
        _check(db, bq.float().numpy(), bt.float().numpy(), what + " bf16")
        assert torch.equal(_bits(DF.pairwise_sqdist(_strided(bq, 3, dev), _strided(bt, 1, dev), ksplit=ksplit)), _bits(db))
        # xq is xt
        xd = xt.to(dev)
        ds = DF.pairwise_sqdist(xd, ksplit=ksplit)
        _check(ds, xt.numpy(), xt.numpy(), what + " xq is xt")
        assert torch.equal(_bits(DF.pairwise_sqdist(xd, xd, ksplit=ksplit)), _bits(ds))
    assert rz.count == 2 + 6


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_integer_rows_are_exact(dtype, dev):
    """integers in -8..8: every product and every sum is an integer below 2^53, so any order of summation gives the integer result"""
    from dcpt_amd import functional as DF

    rs = np.random.RandomState(20372)
    q, t = rs.randint(-8, 9, (20, 256)), rs.randint(-8, 9, (37, 256))
    want = ((q[:, None, :] - t[None, :, :]) ** 2).sum(-1).astype(np.float64)
    for ksplit in (0, 1, 3, 64):
        d2 = DF.pairwise_sqdist(torch.from_numpy(q).to(dtype).to(dev), torch.from_numpy(t).to(dtype).to(dev), ksplit=ksplit).cpu().numpy()
        wrong = int((d2 != want).sum())
        print(f"integer rows (20, 37, 256) {dtype} ksplit {ksplit}: {wrong} of {want.size} entries differ from the integer result")
        assert wrong == 0
    x = torch.from_numpy(t).to(dtype).to(dev)
    ds = DF.pairwise_sqdist(x, ksplit=2).cpu().numpy()
    assert np.array_equal(ds, ((t[:, None, :] - t[None, :, :]) ** 2).sum(-1).astype(np.float64)) and bool((np.diag(ds) == 0).all())


@pytest.mark.parametrize("Nq,Nt,D,ksplit", [(17, 33, 130, 3), (70, 131, 300, 2)])
def test_an_entry_depends_on_its_two_rows_alone(Nq, Nt, D, ksplit, dev):
    """at a fixed ksplit: permuted rows of xt give permuted columns, a duplicated row equal bits, a sub-block of rows the bits of the full
    call, two runs the same bits -- fp32 and bf16"""
    from dcpt_amd import functional as DF

    for dtype in (torch.float32, torch.bfloat16):
        xq = keyed_input(f"gpuknn.c.{Nq}.q", (Nq, D), lo=2.9, hi=3.1).to(dtype).to(dev)
        xt = keyed_input(f"gpuknn.c.{Nt}.t", (Nt, D), lo=2.9, hi=3.1).to(dtype).to(dev)
        xt[Nt - 1] = xt[2]                                     # a duplicated row, in another tile where there is one
        full = DF.pairwise_sqdist(xq, xt, ksplit=ksplit)
        assert torch.equal(_bits(DF.pairwise_sqdist(xq, xt, ksplit=ksplit)), _bits(full))
        assert torch.equal(_bits(full[:, Nt - 1]), _bits(full[:, 2]))
        perm = torch.from_numpy(np.random.RandomState(Nt).permutation(Nt)).to(dev)
        assert torch.equal(_bits(DF.pairwise_sqdist(xq, xt[perm].contiguous(), ksplit=ksplit)), _bits(full[:, perm]))
        qperm = torch.from_numpy(np.random.RandomState(Nq).permutation(Nq)).to(dev)
        assert torch.equal(_bits(DF.pairwise_sqdist(xq[qperm].contiguous(), xt, ksplit=ksplit)), _bits(full[qperm]))
        # a sub-block: views of the same memory (other base addresses, the same leading dimensions) and copies of it
        sub = DF.pairwise_sqdist(xq[3:9], xt[5:20], ksplit=ksplit)
        assert torch.equal(_bits(sub), _bits(full[3:9, 5:20]))
        assert torch.equal(_bits(DF.pairwise_sqdist(xq[3:9].clone(), xt[5:20].clone(), ksplit=ksplit)), _bits(sub))
        one = DF.pairwise_sqdist(xq[Nq - 1:], xt[Nt - 2:Nt - 1], ksplit=ksplit)
        assert torch.equal(_bits(one), _bits(full[Nq - 1:, Nt - 2:Nt - 1]))


def test_refusals_of_the_python_ops(dev):
    from dcpt_amd import functional as DF

    x = keyed_input("gpuknn.bad", (6, 40)).to(dev)
    with pytest.raises(ValueError, match="contiguous rows"):
        DF.pairwise_sqdist(x.t())
    with pytest.raises(ValueError, match="contiguous rows"):
        DF.pairwise_sqdist(x[:, ::2])
    with pytest.raises(ValueError, match="share"):
        DF.pairwise_sqdist(x, x.to(torch.bfloat16))
    with pytest.raises(ValueError, match="share"):
        DF.pairwise_sqdist(x, x[:, :20].contiguous())
    with pytest.raises(ValueError, match="ksplit"):
        DF.pairwise_sqdist(x, ksplit=11)
    with pytest.raises(ValueError, match="out"):
        DF.pairwise_sqdist(x, out=torch.empty((6, 6), device=dev))
    d2 = DF.pairwise_sqdist(x)
    labels = [0, 1, 0, 1, 0, 1]
    with pytest.raises(ValueError, match="outside"):
        DF.knn_vote(d2, labels, [[0, 1, 6]], [[2]], 1)
    with pytest.raises(ValueError, match="outside"):
        DF.knn_vote(d2, labels, [[0, 1, 2]], [[-1]], 1)
    with pytest.raises(ValueError, match="k must"):
        DF.knn_vote(d2, labels, [[0, 1, 2]], [[3]], 4)
    with pytest.raises(ValueError, match="splits"):
        DF.knn_vote(d2, labels, [[0, 1, 2]], [[3], [4]], 1)
    with pytest.raises(ValueError, match="labels"):
        DF.knn_vote(d2, labels[:5], [[0, 1, 2]], [[3]], 1)
    with pytest.raises(Exception, match="float64"):
        DF.knn_vote(d2.float(), labels, [[0, 1, 2]], [[3]], 1)
    # device index tensors are taken as they are (nothing is read back); nested lists and host tensors give the same result
    a = DF.knn_vote(d2, labels, [[0, 1, 2, 4]], [[3, 5]], 3)
    b = DF.knn_vote(d2, torch.tensor(labels, device=dev), torch.tensor([[0, 1, 2, 4]], device=dev), torch.tensor([[3, 5]]), 3)
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and a[0].dtype == torch.int32 and tuple(a[1].shape) == (1, 2, 3)


# ---- the vote -------------------------------------------------------------------------------------------------
def _vote_case(name):
    """(d2 float64 (N, N), labels, train (S, nt), test (S, nq), k): hand-made matrices"""
    rs = np.random.RandomState(sum(map(ord, name)))
    N, nt, nq, S, k, levels, labs = {"equal": (24, 15, 6, 1, 5, 3, (1, 2, 3)), "ties": (30, 20, 10, 2, 4, 50, (1, 2)),
                                      "labels": (30, 20, 10, 1, 5, 6, (-3, 7, 100)), "k1": (12, 6, 4, 1, 1, 4, (-3, 7, 100)),
                                      "knt": (12, 6, 4, 2, 6, 4, (-3, 7, 100)), "nt1": (5, 1, 4, 1, 1, 4, (7, 100)),
                                      "naninf": (40, 25, 12, 3, 7, 5, (-3, 7, 100)), "S3": (50, 33, 17, 3, 5, 8, (1, 2, 3, 4, 5)),
                                      "nt1000": (1100, 1000, 9, 3, 5, 200, (1, 2, 3, 4, 5)), "k32": (100, 70, 5, 1, 32, 30, (-3, 7, 100))}[name]
    d2 = rs.randint(0, levels, (N, N)).astype(np.float64)
    if name in ("ties", "nt1000"):
        d2 += rs.uniform(0, 1e-3, (N, N))                       # distinct distances: only the vote can tie
    if name == "naninf":
        m = rs.uniform(size=(N, N))
        d2[m < 0.25] = np.nan
        d2[(m >= 0.25) & (m < 0.4)] = np.inf
        d2[(m >= 0.4) & (m < 0.5)] = -0.0
        d2[(m >= 0.5) & (m < 0.55)] = -np.inf
        d2[0] = np.nan                                          # a query that sees NaNs only: the lowest positions
    labels = rs.choice(labs, N)
    splits = [rs.permutation(N) for _ in range(S)]
    train = np.stack([p[:nt] for p in splits])
    test = np.stack([p[nt:nt + nq] for p in splits])
    if name == "naninf":
        test[0, 0] = 0
    return d2, labels, train, test, k


@pytest.mark.parametrize("name", ["equal", "ties", "labels", "k1", "knt", "nt1", "naninf", "S3", "nt1000", "k32"])
def test_vote_is_the_restatement_bit_for_bit(name, dev):
    from kernel_trace import kernel_trace

    from dcpt_amd import functional as DF

    d2, labels, train, test, k = _vote_case(name)
    want_pred, want_nbr, want_d = R.knn(d2, labels, train, test, k)
    ties = sum(R.vote_ties(labels, train[s], want_nbr[s]) for s in range(len(train)))
    # a padded copy: the leading dimension is not the row length
    wide = torch.full((d2.shape[0], d2.shape[1] + 5), float("nan"), dtype=torch.float64, device=dev)
    wide[:, :d2.shape[1]] = torch.from_numpy(d2)
    with kernel_trace() as t:
        pred, nbr, nd = DF.knn_vote(wide[:, :d2.shape[1]], torch.from_numpy(labels), torch.from_numpy(train), torch.from_numpy(test), k)
    assert t.counts == {"knn.vote": 1}, t.counts
    pred, nbr, nd = pred.cpu().numpy(), nbr.cpu().numpy(), nd.cpu().numpy()
    print(f"knn_vote {name}: S {len(train)} nq {test.shape[1]} nt {train.shape[1]} k {k}: {int((pred != want_pred).sum())} predictions, "
          f"{int((nbr != want_nbr).any(-1).sum())} neighbour lists differ from the restatement's; {ties} vote ties, "
          f"{int(np.isnan(want_d).sum())} NaN neighbours")
    assert np.array_equal(nbr, want_nbr) and np.array_equal(pred, want_pred)
    assert np.array_equal(nd.view(np.int64), want_d.view(np.int64))           # the distances as stored, NaN and -0 included
    if name in ("ties", "equal", "nt1000"):
        assert ties > 0
    if name == "naninf":
        assert np.isnan(want_d[0, 0]).all() and want_nbr[0, 0].tolist() == list(range(k))


# ---- end to end ---------------------------------------------------------------------------------------------------
def _same_report(got, want):
    assert list(got) == list(want)
    for key, val in want.items():
        if key == "accuracy":
            assert abs(got[key] - val) <= 1e-12
        else:
            assert got[key]["support"] == val["support"] and all(abs(got[key][m] - val[m]) <= 1e-12 for m in ("precision", "recall", "f1-score"))


@pytest.mark.parametrize("name", ["120x17", "60x1000"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_knn_probe_equals_the_restatement(name, dtype, dev):
    """predictions and reports of all five seeds; one distance matrix, one vote launch"""
    from kernel_trace import kernel_trace

    from basicsr.utils import knn_probe

    x, labels = R.clusters(name)
    if dtype == torch.bfloat16:
        x = R.bf16_round(x)
    want = R.probe(x, labels)
    left_out = sum(r["undecidable"] for r in want)
    total = sum(len(r["test"]) for r in want)
    with kernel_trace() as t:
        reports, mean = knn_probe(torch.from_numpy(x).to(dtype).to(dev), labels)
    assert t.counts == {"knn.pdist2_norm": 1, "knn.pdist2_gemm": 1, "knn.pdist2_finish": 1, "knn.vote": 1}, t.counts
    wrong = sum(int((r["pred"] != w["pred"]).sum()) for r, w in zip(reports, want))
    print(f"knn_probe {name} {dtype}: {wrong} of {total} predictions differ from the restatement's, {left_out} undecidable queries left out "
          f"(cap {total // 1000}); accuracies {[round(r['accuracy'], 4) for r in reports]}, vote ties {[w['ties'] for w in want]}")
    assert left_out == 0, "the fixture leaves a query undecidable: choose another seed for it"
    assert [r["seed"] for r in reports] == list(R.SEEDS) and len(reports) == 5
    for r, w in zip(reports, want):
        assert np.array_equal(r["test_idx"], w["test"]) and np.array_equal(r["train_idx"], w["train"])
        assert np.array_equal(r["pred"], w["pred"])
        _same_report(r["report"], w["report"])
        assert r["text"].splitlines()[0].split() == ["precision", "recall", "f1-score", "support"]
    assert abs(mean - float(np.mean([w["report"]["accuracy"] for w in want]))) <= 1e-12


@pytest.mark.parametrize("batch", [1, 3])
def test_feature_taps_give_the_hooked_rows(batch, dev):
    """the matrices of FeatureTaps against plain forward hooks on the same modules with the same batches: row r is image r's map flattened
    in logical NCHW order, bit for bit; four images, so batch 3 ends on a ragged batch"""
    from basicsr.archs.nafnet_arch import NAFNetBaseline
    from basicsr.utils import FeatureTaps, select_hook_modules

    torch.manual_seed(3)
    net = NAFNetBaseline(3, 8, 1, [1, 1, 1, 2], [1, 1, 1, 1]).to(dev).eval()   # (the tiny network of tests/test_gpu_parity.py)
    x = keyed_input("gpuknn.taps", (4, 3, 32, 48)).to(dev)
    seen = []
    handles = [m.register_forward_hook(lambda mod, inp, out: seen.append(out[-1] if isinstance(out, tuple) else out))
               for _, m in select_hook_modules(net, "decoder", 1)]
    want = None
    with torch.no_grad():
        for b0 in range(0, 4, batch):
            seen.clear()
            net(x[b0:b0 + batch], hook=True)
            rows = [o.reshape(o.shape[0], -1).clone() for o in seen]          # the reference's f.reshape(1, -1), per image
            want = rows if want is None else [torch.cat([w, r]) for w, r in zip(want, rows)]
    for h in handles:
        h.remove()
    with FeatureTaps(net, "decoder", 1, rows=4, hook=True) as taps:
        for b0 in range(0, 4, batch):
            taps(x[b0:b0 + batch])
        assert taps.names == ["decoder0.0", "decoder1.0", "decoder2.0", "decoder3.0"] and taps.count == 4
        feats = taps.features
    assert [tuple(f.shape) for f in feats] == [(4, 64 * 4 * 6), (4, 32 * 8 * 12), (4, 16 * 16 * 24), (4, 8 * 32 * 48)]
    for f, w in zip(feats, want):
        assert f.dtype == torch.float32 and f.is_contiguous() and torch.equal(f.view(torch.int32), w.view(torch.int32))
        assert bool(torch.isfinite(f).all()) and float(f.abs().max()) > 0
    assert not any(m._forward_hooks for m in net.modules())
    with FeatureTaps(net, "decoder", 1, rows=2, hook=True) as taps:
        with pytest.raises(RuntimeError, match="does not fit"):
            taps(x[:3])


def test_the_command_on_the_shipped_option(tmp_path, dev):
    """basicsr/knn.py on options/knn/knn_NAFNet_5d.yml with its synthetic sets (12 images of 32 x 32 each, the three decoder groups): the
    JSON equals the restatement applied to the features the command saved"""
    from basicsr.knn import knn_pipeline

    force = [f"datasets:test_{i}:{k}={v}" for i in range(1, 6) for k, v in (("max_per_set", 12), ("size", 32))]
    knn_pipeline(ROOT, ["-opt", os.path.join(ROOT, "options", "knn", "knn_NAFNet_5d.yml"), "--out", str(tmp_path), "--force_yml", *force,
                        "knn:save_features=true", "knn:hook_depth=0", "knn:batch_size=16"])
    rep = json.load(open(tmp_path / "knn_report.json"))
    labels = np.load(tmp_path / "lr_labels.npy")
    assert rep["n"] == 60 and rep["labels"] == [1, 2, 3, 4, 5] and labels.tolist() == [i for i in range(1, 6) for _ in range(12)]
    assert [lv["module"] for lv in rep["levels"]] == ["decoder0", "decoder1", "decoder2"]
    assert [lv["D"] for lv in rep["levels"]] == [128 * 8 * 8, 64 * 16 * 16, 32 * 32 * 32]
    for lv in rep["levels"]:
        f = np.load(tmp_path / f"lr_features_{lv['level']}.npy")
        assert f.shape == (60, lv["D"]) and f.dtype == np.float32 and np.isfinite(f).all()
        want = R.probe(f, labels)
        left_out = sum(w["undecidable"] for w in want)
        wrong = sum(int((np.array(s["pred"]) != w["pred"]).sum()) for s, w in zip(lv["seeds"], want))
        print(f"basicsr/knn.py level {lv['level']} ({lv['module']}, D = {lv['D']}): {wrong} of 100 predictions differ from the restatement's, "
              f"{left_out} undecidable; mean accuracy {lv['mean_accuracy']:.4f}")
        assert left_out == 0 and wrong == 0
        for s, w in zip(lv["seeds"], want):
            assert s["seed"] == w["seed"] and s["test_idx"] == w["test"].tolist()
            _same_report(s["report"], w["report"])
        assert abs(lv["mean_accuracy"] - float(np.mean([w["report"]["accuracy"] for w in want]))) <= 1e-12
