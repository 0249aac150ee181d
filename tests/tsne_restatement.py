"""Exact t-SNE restated in float64 numpy from the rules of include/dcpt_hip.h (those of scikit-learn's method="exact") and nothing else:
no kernel, no product module.  tests/test_tsne_cpu.py checks every function against scikit-learn's private functions and a recorded golden
file; tests/test_gpu_tsne.py compares the kernels with it."""
import numpy as np

EPS = 2.0 ** -52          # scikit-learn's MACHINE_EPSILON
TOL, MAX_STEPS = 1e-5, 100


def cond_affinities(d2, perplexity):
    """(a): -> pcond (N, N), beta (N,), steps (N,), margin = the smallest | |e| - 1e-5 | over every visited step of every row (the
    step counts of two evaluations are comparable only while that is well above their rounding)"""
    d2 = np.asarray(d2, dtype=np.float64)
    N = d2.shape[0]
    pcond, betas, steps = np.zeros((N, N)), np.zeros(N), np.zeros(N, dtype=np.int32)
    logp, margin = np.log(perplexity), np.inf
    for i in range(N):
        d = np.delete(d2[i], i)
        beta, lo, hi = 1.0, -np.inf, np.inf
        for l in range(MAX_STEPS):
            p = np.exp(-d * beta)
            s = p.sum()
            if s == 0.0:
                s = 1e-8
            p = p / s
            sd = (d * p).sum()
            e = np.log(s) + beta * sd - logp
            margin = min(margin, abs(abs(e) - TOL))
            if abs(e) <= TOL:
                break
            if e > 0.0:
                lo = beta
                beta = beta * 2.0 if hi == np.inf else (beta + hi) / 2.0
            else:
                hi = beta
                beta = beta / 2.0 if lo == -np.inf else (beta + lo) / 2.0
        pcond[i] = np.insert(p, i, 0.0)
        betas[i], steps[i] = beta, l
    return pcond, betas, steps, margin


def joint(pcond):
    """(b)"""
    P = pcond + pcond.T
    np.fill_diagonal(P, 0.0)
    S = max(P.sum(), EPS)
    P = np.maximum(P / S, EPS)
    np.fill_diagonal(P, 0.0)
    return P


def kl_grad(P, Y, exaggeration=1.0):
    """the evaluation of (c) at Y: -> kl, g (N, 2), and the sums of the absolute terms of both (kl_abs scalar, g_abs (N, 2)) that the
    derived bounds of the GPU tests are made of"""
    N = Y.shape[0]
    off = ~np.eye(N, dtype=bool)
    diff = Y[:, None, :] - Y[None, :, :]
    w = 1.0 / (1.0 + (diff ** 2).sum(-1))
    w[~off] = 0.0
    Z = w.sum()
    Q = np.maximum(w / Z, EPS)
    Pe = exaggeration * P
    c = np.where(off, (Pe - Q) * w, 0.0)
    terms = c[:, :, None] * diff
    g = 4.0 * terms.sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(off & (Pe != 0.0), Pe * np.log(np.maximum(Pe, EPS) / Q), 0.0)
    # a relative error r of Z moves every Q by r: each gradient term by about |Q w diff| r, each KL term by about |Pe| r
    g_abs = 4.0 * (np.abs(terms).sum(1) + (np.where(off, Q * w, 0.0)[:, :, None] * np.abs(diff)).sum(1))
    kl_abs = np.abs(t).sum() + np.abs(np.where(off, Pe, 0.0)).sum()
    return t.sum(), g, kl_abs, g_abs


def step(P, Y, update, gains, exaggeration, momentum, lr, min_gain=0.01):
    """one iteration of (c): -> Y, update, gains (new arrays), kl at the old Y, the norm of the gain-scaled gradient, the plain gradient"""
    kl, g, _, _ = kl_grad(P, Y, exaggeration)
    inc = update * g < 0.0
    gains = np.maximum(np.where(inc, gains + 0.2, gains * 0.8), min_gain)
    gs = g * gains
    update = momentum * update - lr * gs
    return Y + update, update, gains, kl, np.sqrt((gs ** 2).sum()), g


def steps(P, Y, update, gains, n, exaggeration, momentum, lr, min_gain=0.01):
    kl = gn = np.nan
    for _ in range(n):
        Y, update, gains, kl, gn, _ = step(P, Y, update, gains, exaggeration, momentum, lr, min_gain)
    return Y, update, gains, kl, gn


def pca_init(d2):
    """classical MDS of the squared distances = PCA of the rows: the two largest eigenpairs of B = -1/2 J d2 J, Y = V sqrt(lambda), each
    column's largest-magnitude entry made positive, scaled so that std(Y[:, 0]) = 1e-4"""
    d2 = np.asarray(d2, dtype=np.float64).copy()
    np.fill_diagonal(d2, 0.0)
    d2 = (d2 + d2.T) / 2.0
    N = d2.shape[0]
    J = np.eye(N) - np.full((N, N), 1.0 / N)
    lam, V = np.linalg.eigh(-0.5 * J @ d2 @ J)
    Y = V[:, [-1, -2]] * np.sqrt(np.maximum(lam[[-1, -2]], 0.0))
    for c in range(2):
        if Y[np.argmax(np.abs(Y[:, c])), c] < 0.0:
            Y[:, c] = -Y[:, c]
    return Y / np.std(Y[:, 0]) * 1e-4


def random_init(N, seed):
    return 1e-4 * np.random.RandomState(seed).standard_normal((N, 2))


def schedule(P, Y, early_exaggeration=12.0, learning_rate="auto", max_iter=2000, n_iter_without_progress=300, min_grad_norm=1e-7,
             check=50, exploration=250):
    """scikit-learn's two-phase schedule on `step`: -> Y, kl, n_iter, history [(iteration, error, grad_norm)]"""
    N = Y.shape[0]
    lr = max(N / early_exaggeration / 4.0, 50.0) if learning_rate == "auto" else float(learning_rate)
    assert max_iter >= exploration   # (scikit-learn refuses less)
    history = []

    def descend(Y, start, last, ex, mom, patience):
        # scikit-learn's _gradient_descent: the error is looked at every `check` iterations and at the last one
        update, gains = np.zeros_like(Y), np.ones_like(Y)
        best, best_it, i, kl = np.finfo(np.float64).max, start, start, np.finfo(np.float64).max
        for i in range(start, last):
            Y, update, gains, e, gn, _ = step(P, Y, update, gains, ex, mom, lr)
            checks = (i + 1) % check == 0
            if checks or i == last - 1:
                kl = e
            if checks:
                history.append((i, e, gn))
                if e < best:
                    best, best_it = e, i
                elif i - best_it > patience:
                    break
                if gn <= min_grad_norm:
                    break
        return Y, kl, i

    Y, kl, it = descend(Y, 0, exploration, early_exaggeration, 0.5, exploration)
    if it + 1 < max_iter:
        Y, kl, it = descend(Y, it + 1, max_iter, 1.0, 0.8, n_iter_without_progress)
    return Y, kl, it, history


def neighbour_purity(Y, labels, k=5):
    """the share of each point's k nearest embedding neighbours that carry its label, averaged"""
    labels = np.asarray(labels)
    d = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    nn = np.argsort(d, axis=1, kind="stable")[:, :k]
    return float((labels[nn] == labels[:, None]).mean())


def blobs(N, D, centers, seed, spread=1.0, sep=10.0):
    """seeded Gaussian blobs -> (X float64 (N, D), labels); point i belongs to blob i % centers"""
    rs = np.random.RandomState(seed)
    mu = sep * rs.standard_normal((centers, D))
    labels = np.arange(N) % centers
    return mu[labels] + spread * rs.standard_normal((N, D)), labels


def sqdist32(X):
    """squared distances of the rows, rounded to float32 VALUES and returned as float64 with a zero diagonal: scikit-learn, the
    restatement and the kernels then see the same numbers"""
    X = np.asarray(X, dtype=np.float64)
    d = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    d = d.astype(np.float32).astype(np.float64)
    d = np.maximum(d, d.T)
    np.fill_diagonal(d, 0.0)
    return d


# ---- the shared cases of tests/test_tsne_cpu.py, tests/test_gpu_tsne.py and tools/make_golden_tsne.py ---------------------------------
# name -> (N, perplexity, kind, seed); kinds: "blobs"; "dup": rows 3..5 repeat rows 0..2 (zero off-diagonal distances); "far": the rows
# scaled by 200, every distance above 1e5, so that exp(-d2) is 0 for all of them and s == 0 at beta = 1
AFFINITY_CASES = {
    "n2": (2, 1.5, "blobs", 0), "n3": (3, 1.5, "blobs", 0), "n37": (37, 5.0, "blobs", 0), "n63": (63, 30.0, "blobs", 1),
    "n64": (64, 30.0, "blobs", 0), "n65": (65, 30.0, "blobs", 1), "n150": (150, 30.0, "blobs", 0), "n257": (257, 30.0, "blobs", 2),
    "n1030": (1030, 30.0, "blobs", 2), "dup": (70, 30.0, "dup", 0), "far": (66, 30.0, "far", 0),
}
GOLDEN_CASES = ("n2", "n3", "n37", "n63", "n64", "n65", "n150", "dup", "far")   # N <= 150: recorded from scikit-learn
# The seeds are chosen for the margin: with seed 0 the cases n65, n257 and n1030 came within 1.2e-9 .. 1.7e-9 of the tolerance; with the
# seeds above the smallest margin of any case is 2.2e-8 (n1030), seven orders above the rounding of e.
MARGIN = 1e-9   # every visited | |e| - 1e-5 | of a case must exceed this for its step counts to be comparable


def case_d2(name):
    N, perplexity, kind, seed = AFFINITY_CASES[name]
    X, labels = blobs(N, 16, min(5, N), 1000 + seed)
    if kind == "dup":
        X[3:6] = X[0:3]
    if kind == "far":
        X = 200.0 * X
    return sqdist32(X), perplexity


def case_y(N, seed, scale):
    """the "random" rule's draw, scaled: 1e-4 is the rule itself, 1 and 1e3 visit the middle and the far regime of w"""
    return scale * np.random.RandomState(seed).standard_normal((N, 2))

TEN_STEP_CASES = ("n37", "n150")        # ten iterations from the "random" start (seed 3)
TEN_STEP_PARAMS = (12.0, 0.5, 50.0)     # exaggeration, momentum, lr: the first phase of the schedule at N <= 2400


def driver_data():
    """the whole-driver case: 150 points, five separated blobs in 50 dimensions -> (X float32, labels, the float64 squared distances of
    the unit-length float32 rows, rounded to float32 values)"""
    X, labels = blobs(150, 50, 5, 77)
    X = X.astype(np.float32)
    U = X / np.sqrt((X * X).sum(1, keepdims=True, dtype=np.float32))
    return X, labels, sqdist32(U.astype(np.float64))
