"""Kernel-blind numpy restatement of the kNN degradation probe (include/dcpt_hip.h dcpt_pdist2_fwd, dcpt_knn_vote_fwd; basicsr/utils/knn_probe.py):
the yardstick of tests/test_knn_cpu.py and tests/test_gpu_knn.py.  Nothing here knows how the kernels sum.

* distances: T_ij = sum_k (q_ik - t_jk)^2 in ``longdouble``, each difference formed in longdouble from the fp32 / bf16-rounded values.
* neighbours: a stable argsort of the distances of a query's training columns -- ascending (distance, position), a NaN after every number.
* vote: the label with the largest count among the k neighbours, the smallest label on equal counts.
* the split rule of scikit-learn's ``train_test_split`` and the report of its ``classification_report``, written out again here (not
  imported from the product); tests/test_knn_cpu.py compares both with scikit-learn where it is installed.
* ``error_bound``: E_ij = 4 D 2^-53 (|q_i|^2 + |t_j|^2), the derived bound of the issue -- products exact, an fp64 sum of D terms in any order
  errs by at most D 2^-53 sum |terms|, sum |q_k t_k| <= (n + m) / 2, three such sums and three final roundings: (2 D + 3) 2^-53 (n + m).
* ``decidable``: a query whose first k + 1 restated distances have adjacent gaps all above 2 max E of its row cannot change its
  neighbour list (or its order) under an error of E per entry."""
import math

import numpy as np

SEEDS = (0, 223, 929, 1234, 10086)
FIXTURES = {"500x64": (500, 64), "120x17": (120, 17), "60x1000": (60, 1000)}   # (N, D) of the seeded Gaussian clusters


def clusters(name, classes=5):
    """the fixture: N fp32 rows of D values, class c (label c + 1, as the reference's 1..5) a Gaussian cloud around its own seeded centre;
    returns (x float32 (N, D), labels int64 (N,))"""
    n, d = FIXTURES[name]
    rng = np.random.RandomState(1000 + n + d)
    centres = rng.normal(0.0, 1.0, (classes, d))
    labels = np.arange(n) % classes
    x = centres[labels] * (2.0 / math.sqrt(d)) + rng.normal(0.0, 1.0, (n, d))
    return x.astype(np.float32), labels.astype(np.int64) + 1


def bf16_round(x):
    """fp32 values rounded to bf16 (nearest even), returned as fp32"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def sqdist(xq, xt):
    """T (Nq, Nt) longdouble: sum_k (q_ik - t_jk)^2 (in blocks of rows, to bound the memory; ``xq is xt``: one triangle, mirrored)"""
    q, t = np.asarray(xq).astype(np.longdouble), np.asarray(xt).astype(np.longdouble)
    block = max(1, int(math.sqrt(4e6 / q.shape[1])))
    out = np.empty((q.shape[0], t.shape[0]), dtype=np.longdouble)
    for i0 in range(0, q.shape[0], block):
        for j0 in range(0, t.shape[0], block):
            if xq is xt and j0 < i0:
                out[i0:i0 + block, j0:j0 + block] = out[j0:j0 + block, i0:i0 + block].T   # ((a - b)^2 == (b - a)^2 exactly)
                continue
            d = q[i0:i0 + block, None, :] - t[None, j0:j0 + block, :]
            out[i0:i0 + block, j0:j0 + block] = (d * d).sum(-1)
    return out


def error_bound(xq, xt):
    """E (Nq, Nt) float64 = 4 D 2^-53 (|q_i|^2 + |t_j|^2)"""
    q, t = np.asarray(xq).astype(np.longdouble), np.asarray(xt).astype(np.longdouble)
    n, m = (q * q).sum(-1), (t * t).sum(-1)
    return (4.0 * q.shape[1] * 2.0 ** -53 * (n[:, None] + m[None, :])).astype(np.float64)


def neighbours(d_row, k):
    """positions of the k nearest of one query's candidate distances: ascending (distance, position), NaN last"""
    return np.argsort(np.asarray(d_row), kind="stable")[:k]


def vote(neigh_labels):
    """the majority label; the smallest label among equal counts"""
    vals, counts = np.unique(np.asarray(neigh_labels), return_counts=True)
    return vals[np.argmax(counts)]   # (np.unique sorts ascending; argmax takes the first maximum)


def knn(d2, labels, train_idx, test_idx, k):
    """(pred (S, nq), nbr (S, nq, k), nbr_d2 (S, nq, k)) for S splits over one distance matrix: ``train_idx[s]`` its columns, ``test_idx[s]``
    its rows, ``labels[c]`` the label of column c"""
    d2, labels = np.asarray(d2), np.asarray(labels)
    train_idx, test_idx = np.asarray(train_idx), np.asarray(test_idx)
    S, nq = test_idx.shape
    pred = np.empty((S, nq), dtype=np.int64)
    nbr = np.empty((S, nq, k), dtype=np.int64)
    nd = np.empty((S, nq, k), dtype=d2.dtype)
    for s in range(S):
        for q in range(nq):
            row = d2[test_idx[s, q]][train_idx[s]]
            pos = neighbours(row, k)
            nbr[s, q], nd[s, q] = pos, row[pos]
            pred[s, q] = vote(labels[train_idx[s][pos]])
    return pred, nbr, nd


def vote_ties(labels, train_idx, nbr):
    """how many queries of one split had two labels with the same, largest count"""
    n = 0
    for pos in nbr:
        _, counts = np.unique(np.asarray(labels)[np.asarray(train_idx)[pos]], return_counts=True)
        n += int((counts == counts.max()).sum() > 1)
    return n


def decidable(T, E, train_idx, test_idx, k):
    """bool (nq,) of one split: every adjacent gap among the query's first k + 1 restated distances exceeds 2 max E of its row"""
    ok = np.empty(len(test_idx), dtype=bool)
    for q, r in enumerate(test_idx):
        row = np.sort(T[r][train_idx].astype(np.float64), kind="stable")[:k + 1]
        ok[q] = bool(np.all(np.diff(row) > 2.0 * float(E[r][train_idx].max())))
    return ok


def train_test_indices(n, test_size, seed):
    n_test = int(math.ceil(test_size * n))
    perm = np.random.RandomState(seed).permutation(n)
    return perm[n_test:], perm[:n_test]


def report(y_true, y_pred):
    """the dict of scikit-learn's classification_report(output_dict=True); a zero denominator gives 0"""
    y_true, y_pred = np.asarray(y_true), np.asarray(y_pred)
    out, rows = {}, []
    for lab in np.unique(np.concatenate([y_true, y_pred])):
        tp = float(np.sum((y_true == lab) & (y_pred == lab)))
        nt, npred = float(np.sum(y_true == lab)), float(np.sum(y_pred == lab))
        p, r = (tp / npred if npred else 0.0), (tp / nt if nt else 0.0)
        f = 2 * tp / (nt + npred) if nt + npred else 0.0
        out[str(lab)] = {"precision": p, "recall": r, "f1-score": f, "support": int(nt)}
        rows.append(out[str(lab)])
    total = int(y_true.size)
    out["accuracy"] = float(np.sum(y_true == y_pred)) / total
    sup = np.array([r["support"] for r in rows], dtype=np.float64)
    for name, w in (("macro avg", np.ones(len(rows))), ("weighted avg", sup)):
        out[name] = {k: float(np.sum(w * np.array([r[k] for r in rows])) / np.sum(w)) for k in ("precision", "recall", "f1-score")}
        out[name]["support"] = total
    return out


def probe(x, labels, k=5, test_size=0.33, seeds=SEEDS):
    """the whole probe on the host: per seed (train, test, pred, nbr, report, undecidable count), from the longdouble distances"""
    T = sqdist(x, x)
    E = error_bound(x, x)
    out = []
    for seed in seeds:
        train, test = train_test_indices(len(x), test_size, seed)
        pred, nbr, _ = knn(T, labels, train[None], test[None], k)
        ok = decidable(T, E, train, test, k)
        out.append({"seed": seed, "train": train, "test": test, "pred": pred[0], "nbr": nbr[0], "report": report(np.asarray(labels)[test], pred[0]),
                    "undecidable": int((~ok).sum()), "ties": vote_ties(labels, train, nbr[0])})
    return out
