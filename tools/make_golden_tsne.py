"""Record scikit-learn's exact t-SNE on the CPU cases of tests/tsne_restatement.py into tests/golden/tsne.npz, so that tests/test_tsne_cpu.py
runs where scikit-learn is absent:

    python tools/make_golden_tsne.py

Per case of GOLDEN_CASES (N <= 150): ``P_<case>`` from ``_joint_probabilities`` (the distances are float32 values, so its rounding changes
nothing), ``kl_<case>`` / ``grad_<case>`` from ``_kl_divergence`` at the case's Y (scale 1) with exaggeration 1.  Per ten-step case:
``y10_<case>`` from ``_gradient_descent`` with float64 parameters, and it prints the relative difference between that and the
restatement -- the number the GPU test's ten-step tolerance is 1000 times of (tests/test_gpu_tsne.py TEN_STEP_CPU_DIFF)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tsne_restatement as R  # noqa: E402


def sklearn_ten_steps(P, Y0, exaggeration, momentum, lr, n=10):
    from scipy.spatial.distance import squareform
    from sklearn.manifold import _t_sne as T

    N = Y0.shape[0]
    p, _, _ = T._gradient_descent(T._kl_divergence, Y0.ravel().copy(), it=0, max_iter=n, n_iter_check=50, momentum=momentum,
                                  learning_rate=lr, args=[squareform(exaggeration * P, checks=False), 1.0, N, 2])
    return p.reshape(N, 2)


def main():
    from scipy.spatial.distance import squareform
    from sklearn.manifold import _t_sne as T
    import sklearn

    out = {"sklearn_version": np.array(sklearn.__version__)}
    for name in R.GOLDEN_CASES:
        d2, perplexity = R.case_d2(name)
        N = d2.shape[0]
        Pc = T._joint_probabilities(d2.astype(np.float32), perplexity, 0)
        out[f"P_{name}"] = squareform(Pc)
        Y = R.case_y(N, 7, 1.0)
        kl, grad = T._kl_divergence(Y.ravel().copy(), Pc, 1.0, N, 2)
        out[f"kl_{name}"], out[f"grad_{name}"] = np.array(kl), grad.reshape(N, 2)
    for name in R.TEN_STEP_CASES:
        d2, perplexity = R.case_d2(name)
        N = d2.shape[0]
        P = R.joint(R.cond_affinities(d2, perplexity)[0])
        Y0 = R.random_init(N, 3)
        want = sklearn_ten_steps(P, Y0, *R.TEN_STEP_PARAMS)
        got = R.steps(P, Y0, np.zeros_like(Y0), np.ones_like(Y0), 10, *R.TEN_STEP_PARAMS)[0]
        print(f"{name}: ten steps, restatement vs scikit-learn: {np.abs(got - want).max() / np.abs(want).max():.3e} of the largest coordinate")
        out[f"y10_{name}"] = want
    path = os.path.join(ROOT, "tests", "golden", "tsne.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
