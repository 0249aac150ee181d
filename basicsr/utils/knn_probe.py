"""The kNN degradation probe (the reference's ``knn_gen.py`` + ``knn.py``): how well do an encoder's decoder features tell the degradations
apart?  The reference flattens the hooked feature maps per image, dumps them to ``.npy`` and fits scikit-learn's
``KNeighborsClassifier(5)`` over five seeded 67/33 splits on the host.  Here the features stay on the device: ``FeatureTaps`` writes them
into one (N, D) matrix per hook level, ``dcpt_amd.functional.pairwise_sqdist`` makes ONE fp64 distance matrix of it with itself on the fp64
matrix cores, ``knn_vote`` finds the neighbours and votes for all seeds in one launch, and the predictions come back in one transfer.
scikit-learn is not a dependency: ``train_test_indices`` and ``classification_report`` restate its split rule and its report."""
from __future__ import annotations

import math

import numpy as np
import torch

__all__ = ["select_hook_modules", "FeatureTaps", "train_test_indices", "classification_report", "knn_probe", "KNN_SEEDS"]

KNN_SEEDS = (0, 223, 929, 1234, 10086)   # the reference's knn.py:14


def select_hook_modules(net, hook_names, hook_depth=1):
    """[(name, module)] of the bare ``net`` that the taps hook.  ``hook_depth`` 1 (default) is the reference's rule
    (degradation_classification_pretrain_model.py:65-68): ``hook_names in name and name.count(".") == 1``.  ``hook_depth`` 0 takes the
    direct children whose name contains ``hook_names``, containers (ModuleList / ModuleDict) left out: what the reference's rule selects
    on its DDP-wrapped net, where ``module.decode_layers0`` has one dot -- SwinIR's decoder RSTBs, attributes of the net itself, which the
    published multi-GPU runs tapped (on the bare net the one-dot rule picks their never-called ``residual_group`` / ``conv`` children
    instead)."""
    if hook_names is None:
        raise ValueError("hook_names is required (e.g. 'decoder' for NAFNet, 'decoder_level' for Restormer)")
    if hook_depth not in (0, 1):
        raise ValueError(f"hook_depth must be 0 or 1, got {hook_depth!r}")
    if hook_depth == 0:
        return [(name, m) for name, m in net.named_children()
                if hook_names in name and not isinstance(m, (torch.nn.ModuleList, torch.nn.ModuleDict))]
    # reference :65-68 (it walks the wrapped net, whose names gain a "module." prefix under DDP and then never match)
    return [(name, m) for name, m in net.named_modules() if hook_names in name and name.count(".") == 1]


class FeatureTaps:
    """Forward hooks on the modules ``select_hook_modules(net, hook_names, hook_depth)`` picks.  ``taps(x)`` runs ``net`` on a batch under
    ``no_grad`` and writes every tapped map (a tuple output's last element), flattened per image in logical NCHW order as the reference's
    ``f.reshape(1, -1)``, into the next rows of one preallocated (rows, D_level) device matrix per hook, of the map's dtype.  The
    matrices are allocated at the first batch, when the maps' sizes are known; ``features`` lists them in the order the hooks fired,
    ``names`` the hooked modules in that order, ``count`` the rows written.  ``net_kwargs`` go to every call of the net (NAFNetBaseline:
    ``hook=True`` skips the ending conv).  ``close()`` removes the hooks; the object is a context manager that does so."""

    def __init__(self, net, hook_names, hook_depth=1, rows=None, **net_kwargs):
        self.net = net
        self.picked = select_hook_modules(net, hook_names, hook_depth)
        if not self.picked:
            raise ValueError(f"no module of the net matches hook_names={hook_names!r} (hook_depth={hook_depth})")
        self.rows = rows
        self.net_kwargs = net_kwargs
        self.features, self.names, self.count = [], [], 0
        self._level = 0
        self._handles = [m.register_forward_hook(self._make_hook(name)) for name, m in self.picked]

    def reserve(self, rows):
        """the number of images the matrices hold; before the first batch"""
        if self.features:
            raise RuntimeError("FeatureTaps.reserve: the matrices are already allocated")
        self.rows = int(rows)

    def _make_hook(self, name):
        def hook(module, inputs, output):
            if isinstance(output, (tuple, list)):
                output = output[-1]
            B = output.shape[0]
            if self._level == len(self.features):
                if self.count:
                    raise RuntimeError(f"FeatureTaps: hook {name} fired {self._level + 1} times in a batch after {len(self.features)} in the first")
                if self.rows is None:
                    raise RuntimeError("FeatureTaps: give `rows` (or call reserve) before the first batch")
                self.features.append(torch.empty((self.rows, output[0].numel()), dtype=output.dtype, device=output.device))
                self.names.append(name)
            mat = self.features[self._level]
            if self.count + B > mat.shape[0] or output[0].numel() != mat.shape[1] or output.dtype != mat.dtype:
                raise RuntimeError(f"FeatureTaps: a map of {tuple(output.shape)} {output.dtype} does not fit rows {self.count}.. of the "
                                   f"{tuple(mat.shape)} {mat.dtype} matrix of hook {self.names[self._level]}")
            mat[self.count:self.count + B].view(output.shape).copy_(output.detach())   # (logical order: the strides are the copy's business)
            self._level += 1
            return None
        return hook

    def __call__(self, x):
        self._level = 0
        with torch.no_grad():
            self.net(x, **self.net_kwargs)
        if self._level != len(self.features) or not self.features:
            raise RuntimeError(f"FeatureTaps: {self._level} hooks fired, {len(self.features)} in the first batch (modules {self.names})")
        self.count += x.shape[0]
        return self.features

    def close(self):
        for h in self._handles:
            h.remove()
        self._handles = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def train_test_indices(n, test_size=0.33, seed=0):
    """``(train, test)`` index arrays of scikit-learn's ``train_test_split(range(n), test_size=test_size, random_state=seed)`` (shuffled, not
    stratified): n_test = ceil(test_size n), n_train = n - n_test, ``perm = np.random.RandomState(seed).permutation(n)``, test =
    ``perm[:n_test]``, train = ``perm[n_test:]``."""
    n = int(n)
    if not 0.0 < float(test_size) < 1.0:
        raise ValueError(f"test_size must lie in (0, 1), got {test_size!r}")
    n_test = int(math.ceil(test_size * n))
    n_train = n - n_test
    if n_train < 1 or n_test < 1:
        raise ValueError(f"{n} samples at test_size={test_size} leave an empty train or test set")
    perm = np.random.RandomState(seed).permutation(n)
    return perm[n_test:], perm[:n_test]


def _div(a, b):
    return float(a) / float(b) if b else 0.0


def classification_report(y_true, y_pred, digits=2):
    """``(report, text)`` of scikit-learn's ``classification_report``: ``report`` has the keys of ``output_dict=True`` -- per label (as
    ``str(label)``, the labels of ``y_true`` and ``y_pred`` together, ascending) ``precision`` / ``recall`` / ``f1-score`` / ``support``,
    then ``accuracy``, ``macro avg`` and ``weighted avg`` -- and ``text`` is the table in scikit-learn's layout.  precision = tp / (tp + fp),
    recall = tp / (tp + fn), f1 = 2 tp / (2 tp + fp + fn); a zero denominator gives 0."""
    y_true, y_pred = np.asarray(y_true).reshape(-1), np.asarray(y_pred).reshape(-1)
    if y_true.shape != y_pred.shape or y_true.size == 0:
        raise ValueError(f"classification_report: y_true {y_true.shape} and y_pred {y_pred.shape} must be two non-empty lists of one length")
    labels = np.unique(np.concatenate([y_true, y_pred]))
    report, rows = {}, []
    for lab in labels:
        tp = int(np.sum((y_true == lab) & (y_pred == lab)))
        n_true, n_pred = int(np.sum(y_true == lab)), int(np.sum(y_pred == lab))
        row = {"precision": _div(tp, n_pred), "recall": _div(tp, n_true), "f1-score": _div(2 * tp, n_true + n_pred), "support": n_true}
        report[str(lab)] = row
        rows.append(row)
    total = int(y_true.size)
    report["accuracy"] = _div(int(np.sum(y_true == y_pred)), total)
    keys = ("precision", "recall", "f1-score")
    report["macro avg"] = {**{k: float(np.mean([r[k] for r in rows])) for k in keys}, "support": total}
    report["weighted avg"] = {**{k: _div(np.sum([r[k] * r["support"] for r in rows]), total) for k in keys}, "support": total}

    names = [str(lab) for lab in labels]
    width = max(max(len(n) for n in names), len("weighted avg"), digits)
    text = "{:>{w}s} ".format("", w=width) + "".join(" {:>9}".format(h) for h in (*keys, "support")) + "\n\n"
    fmt = "{:>{w}s} " + " {:>9.{d}f}" * 3 + " {:>9}\n"
    for n in names:
        r = report[n]
        text += fmt.format(n, r["precision"], r["recall"], r["f1-score"], r["support"], w=width, d=digits)
    text += "\n"
    text += ("{:>{w}s} " + " {:>9}" * 2 + " {:>9.{d}f} {:>9}\n").format("accuracy", "", "", report["accuracy"], total, w=width, d=digits)
    for n in ("macro avg", "weighted avg"):
        r = report[n]
        text += fmt.format(n, r["precision"], r["recall"], r["f1-score"], r["support"], w=width, d=digits)
    return report, text


def knn_probe(features, labels, n_neighbors=5, test_size=0.33, seeds=KNN_SEEDS, ksplit=0):
    """The reference's knn.py on one (N, D) fp32 or bf16 DEVICE matrix of flattened features and N integer labels: for every seed a
    shuffled split (``train_test_indices``), the ``n_neighbors`` nearest training rows of every test row by Euclidean distance and their
    majority label (ties: the nearer-sorted lower position among equal distances, the smallest label among equal counts -- scikit-learn's
    rules), and the classification report of the test rows.  One ``pairwise_sqdist`` of the matrix with itself, one ``knn_vote`` over all
    seeds, one transfer of the predictions.  Returns ``(reports, mean_accuracy)``: per seed a dict ``{"seed", "report", "text", "accuracy",
    "pred", "test_idx", "train_idx"}`` (``report`` / ``text`` of ``classification_report``, the arrays on the host), and the mean of the
    accuracies.  The defaults are the reference's."""
    from dcpt_amd import functional as DF

    labels = np.asarray(labels.cpu() if torch.is_tensor(labels) else labels).reshape(-1).astype(np.int64)
    d2 = DF.pairwise_sqdist(features, ksplit=ksplit)   # (raises for a CPU tensor: there is no host path)
    n = d2.shape[0]
    if labels.size != n:
        raise ValueError(f"knn_probe: {n} feature rows and {labels.size} labels")
    if labels.min() < -(1 << 31) or labels.max() >= (1 << 31):
        raise ValueError("knn_probe: the labels must fit int32")
    splits = [train_test_indices(n, test_size, s) for s in seeds]
    train = np.stack([tr for tr, _ in splits])
    test = np.stack([te for _, te in splits])
    pred, _, _ = DF.knn_vote(d2, torch.from_numpy(labels), torch.from_numpy(train), torch.from_numpy(test), n_neighbors)
    pred = pred.cpu().numpy()   # the one transfer
    reports = []
    for s, seed in enumerate(seeds):
        rep, text = classification_report(labels[test[s]], pred[s])
        reports.append({"seed": int(seed), "report": rep, "text": text, "accuracy": rep["accuracy"], "pred": pred[s].astype(np.int64),
                        "test_idx": test[s], "train_idx": train[s]})
    return reports, float(np.mean([r["accuracy"] for r in reports]))
