"""Exact t-SNE of the probe's features on the device: the reference's ``t_sne.py`` (unit-length rows, ``sklearn.manifold.TSNE(2)``) on the
fp64 kernels of ``dcpt_amd`` (``pairwise_sqdist``, ``tsne_affinities``, ``tsne_steps``).  After one distance call the (N, D) features are
never touched again: the affinities, the descent and the PCA start are all functions of the (N, N) squared distances.  The schedule is
scikit-learn's: 250 iterations with the exaggerated P and momentum 0.5, then momentum 0.8 up to ``max_iter``, the two stopping rules
looked at every 50 iterations.  No scikit-learn import."""
import numpy as np
import torch

CHECK_EVERY, EXPLORATION_ITERS = 50, 250          # scikit-learn's n_iter_check and _EXPLORATION_MAX_ITER
TSNE_LABEL_NAMES = {1: "haze", 2: "motion-blur", 3: "noise", 4: "rain", 5: "low_light"}   # the reference's t_sne.py


def pca_init_from_sqdist(d2):
    """The PCA start without a second pass over the features: classical MDS.  With J = I - 11^t / N the matrix B = -1/2 J d2 J is the
    Gram matrix of the centred rows, so its two largest eigenpairs give the first two principal components' scores V sqrt(lambda).  Each
    column's sign is chosen so that its largest-magnitude entry is positive (a mirrored embedding is the same embedding), and the result is
    scaled so that ``np.std(Y[:, 0]) == 1e-4`` as scikit-learn does.  ``d2``: (N, N) float64 numpy array; its diagonal is taken as 0 and it
    is symmetrised (the device distances promise neither)."""
    d2 = np.array(d2, dtype=np.float64)
    np.fill_diagonal(d2, 0.0)
    d2 = (d2 + d2.T) / 2.0
    row = d2.mean(axis=1, keepdims=True)
    B = -0.5 * (d2 - row - row.T + d2.mean())
    lam, V = np.linalg.eigh(B)
    Y = V[:, [-1, -2]] * np.sqrt(np.maximum(lam[[-1, -2]], 0.0))
    for c in range(2):
        if Y[np.argmax(np.abs(Y[:, c])), c] < 0.0:
            Y[:, c] = -Y[:, c]
    return Y / np.std(Y[:, 0]) * 1e-4


def neighbour_label_share(Y, labels, k=5):
    """the share of each point's ``k`` nearest embedding neighbours that carry its label, averaged over the points"""
    Y, labels = np.asarray(Y, dtype=np.float64), np.asarray(labels).reshape(-1)
    d = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    nn = np.argsort(d, axis=1, kind="stable")[:, :min(k, len(Y) - 1)]
    return float((labels[nn] == labels[:, None]).mean())


def tsne_embed(features=None, d2=None, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto", max_iter=2000,
               n_iter_without_progress=300, min_grad_norm=1e-7, init="pca", seed=0, normalize=True):
    """Exact t-SNE to two dimensions.  ``features``: an (N, D) fp32 / bf16 device tensor (``normalize``: the reference's division of every
    row by its L2 norm, on an fp32 copy on the device), or ``d2``: a float64 (N, N) squared-distance device tensor.  ``init``: "pca"
    (`pca_init_from_sqdist`: one N^2 transfer and a host eigen-decomposition), "random" (``1e-4 RandomState(seed).standard_normal((N, 2))``
    in float64) or an (N, 2) array taken as given.  ``learning_rate="auto"`` is ``max(N / early_exaggeration / 4, 50)``.  The descent runs
    in chunks of 50 iterations on the device; per chunk the KL divergence and the gradient norm come back, nothing else before the final
    embedding.  Returns ``{"embedding": (N, 2) float64 numpy, "kl_divergence", "n_iter", "history": [(iteration, error, grad_norm)]}``:
    ``kl_divergence`` is that of the returned embedding, ``n_iter`` the index of the last iteration run, a history entry the error at the
    embedding before that iteration's move and the norm of its gain-scaled gradient, as scikit-learn logs them."""
    from dcpt_amd import functional as DF

    if (features is None) == (d2 is None):
        raise ValueError("tsne_embed: give either features or d2")
    max_iter = int(max_iter)
    if max_iter < EXPLORATION_ITERS:
        raise ValueError(f"tsne_embed: max_iter must be at least {EXPLORATION_ITERS} (the exploration phase), got {max_iter}")
    if d2 is None:
        x = features
        if normalize:
            if not torch.is_tensor(x) or not x.is_cuda:
                DF.pairwise_sqdist(x)   # (raises the product's no-CPU-path error)
            x = x.detach().float()
            x = x / x.norm(dim=1, keepdim=True)
        d2 = DF.pairwise_sqdist(x)
    N = d2.shape[0]
    P, _, _ = DF.tsne_affinities(d2, perplexity)
    dev = P.device
    if isinstance(init, str):
        if init == "pca":
            Y0 = pca_init_from_sqdist(d2.cpu().numpy())
        elif init == "random":
            Y0 = 1e-4 * np.random.RandomState(seed).standard_normal((N, 2))
        else:
            raise ValueError(f"tsne_embed: init must be 'pca', 'random' or an (N, 2) array, got {init!r}")
    else:
        Y0 = np.array(init.detach().cpu().numpy() if torch.is_tensor(init) else init, dtype=np.float64)
        if Y0.shape != (N, 2):
            raise ValueError(f"tsne_embed: only two output dimensions exist; init must be ({N}, 2), got {Y0.shape}")
    lr = max(N / float(early_exaggeration) / 4.0, 50.0) if learning_rate == "auto" else float(learning_rate)
    Y = torch.from_numpy(np.ascontiguousarray(Y0)).to(dev)
    history = []

    def descend(start, last, exaggeration, momentum, patience):
        # scikit-learn's _gradient_descent: update = 0 and gains = 1 at the start of a phase; the error is looked at every 50 iterations
        # and at the phase's last one, the stopping rules every 50
        update, gains = torch.zeros_like(Y), torch.ones_like(Y)
        best, best_it, i, kl = np.finfo(np.float64).max, start, start, np.finfo(np.float64).max
        while i < last:
            stop = min((i // CHECK_EVERY + 1) * CHECK_EVERY, last)   # the chunk ends with iteration stop - 1
            stats = DF.tsne_steps(P, Y, update, gains, stop - i, exaggeration, momentum, lr).tolist()
            i = stop - 1
            kl = stats[0]
            if stop % CHECK_EVERY == 0:
                history.append((i, stats[0], stats[1]))
                if stats[0] < best:
                    best, best_it = stats[0], i
                elif i - best_it > patience:
                    break
                if stats[1] <= min_grad_norm:
                    break
            i = stop
        return kl, min(i, last - 1) if last > start else start

    kl, it = descend(0, EXPLORATION_ITERS, float(early_exaggeration), 0.5, EXPLORATION_ITERS)
    if it + 1 < max_iter:
        kl, it = descend(it + 1, max_iter, 1.0, 0.8, int(n_iter_without_progress))
    kl = float(DF.tsne_kl(P, Y)[0])   # of the RETURNED embedding (scikit-learn reports the error before the last move: the history's form)
    return {"embedding": Y.cpu().numpy(), "kl_divergence": kl, "n_iter": int(it), "history": history}
