"""``python basicsr/tsne.py -opt <yml>``: the reference's ``t_sne.py`` -- the figure of degradation clusters -- on the HIP path.  The features
are those of the kNN probe: ``-opt FILE`` encodes them with ``basicsr/knn.py``'s own functions (same option files, ``options/knn/``), and
``--features DIR`` loads a dump of ``lr_features_<i>.npy`` / ``lr_labels.npy``.  Per hook level the rows are brought to unit length and
embedded by exact t-SNE on the device (``basicsr.utils.tsne_embed``: fp64 distances, affinities and descent; scikit-learn's schedule).

An optional ``tsne:`` block of the option file holds ``tsne_embed``'s arguments (``perplexity``, ``early_exaggeration``, ``learning_rate``,
``max_iter``, ``n_iter_without_progress``, ``min_grad_norm``, ``init``, ``seed``, ``normalize``) and ``label_names`` (a mapping from label to
name; default the reference's list); without it the defaults apply -- ``max_iter`` 2000 is the reference's value.  ``--perplexity`` and
``--max_iter`` on the command line override the block (``--force_yml`` changes only keys a file already has).

Output in ``results/<name>`` (or ``--out``): ``tsne_<level>.npy`` the (N, 2) embedding, ``tsne.json`` with the KL divergence, the
iteration count and the share of each point's 5 nearest embedding neighbours that carry its label, and, where matplotlib imports,
``tsne_<level>.png``: a plain scatter, one colour per label.  A missing matplotlib costs only the picture.  There is no CPU fallback."""
import argparse
import json
import logging
import os
import sys
from os import path as osp

sys.path.insert(0, osp.abspath(osp.join(osp.dirname(__file__), osp.pardir)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from basicsr.utils import get_root_logger, neighbour_label_share, tsne_embed  # noqa: E402
from basicsr.utils.tsne import TSNE_LABEL_NAMES  # noqa: E402

EMBED_KEYS = ("perplexity", "early_exaggeration", "learning_rate", "max_iter", "n_iter_without_progress", "min_grad_norm", "init", "seed",
              "normalize")


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("-opt", type=str, default=None, help="Path to option YAML file (an option file of basicsr/knn.py).")
    parser.add_argument("--features", type=str, default=None, help="embed a directory of lr_features_<i>.npy / lr_labels.npy instead")
    parser.add_argument("--out", type=str, default=None, help="output directory (default results/<name>)")
    parser.add_argument("--force_yml", nargs="+", default=None, help="overrides of keys the option file has, e.g. knn:batch_size=4")
    parser.add_argument("--perplexity", type=float, default=None, help="overrides tsne.perplexity (default 30)")
    parser.add_argument("--max_iter", type=int, default=None, help="overrides tsne.max_iter (default 2000)")
    args = parser.parse_args(argv)
    if (args.opt is None) == (args.features is None):
        parser.error("give either -opt FILE or --features DIR")
    return args


def embed_kwargs(topt):
    """``tsne_embed``'s arguments out of a ``tsne:`` block; an unknown key is an error, not a silent default"""
    topt = dict(topt or {})
    topt.pop("label_names", None)
    unknown = sorted(set(topt) - set(EMBED_KEYS))
    if unknown:
        raise ValueError(f"tsne: unknown keys {unknown}; known: {list(EMBED_KEYS)} and label_names")
    return topt


def label_names(topt):
    names = dict(TSNE_LABEL_NAMES)
    names.update({int(k): str(v) for k, v in ((topt or {}).get("label_names") or {}).items()})
    return names


def scatter_png(path, Y, labels, names):
    """one colour per label; False where matplotlib is missing"""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        return False
    fig, ax = plt.subplots(figsize=(8, 8))
    for v in sorted({int(x) for x in labels}):
        m = labels == v
        ax.scatter(Y[m, 0], Y[m, 1], s=12, alpha=0.7, label=names.get(v, str(v)))
    ax.legend(title="degradation")
    ax.set_xlabel("tsne-2d-one")
    ax.set_ylabel("tsne-2d-two")
    fig.savefig(path, dpi=150, bbox_inches="tight")
    plt.close(fig)
    return True


def run(features, names, labels, topt, out_dir, logger, name):
    kwargs, lnames = embed_kwargs(topt), label_names(topt)
    os.makedirs(out_dir, exist_ok=True)
    report = {"name": name, "n": int(len(labels)), "labels": sorted({int(v) for v in labels}), "levels": []}
    for lvl, (f, mod) in enumerate(zip(features, names), start=1):
        res = tsne_embed(f, **kwargs)
        Y = res["embedding"]
        np.save(osp.join(out_dir, f"tsne_{lvl}.npy"), Y)
        share = neighbour_label_share(Y, labels, 5)
        png = scatter_png(osp.join(out_dir, f"tsne_{lvl}.png"), Y, labels, lnames)
        logger.info(f"level {lvl} ({mod}, D = {f.shape[1]}): KL {res['kl_divergence']:.4f} after {res['n_iter'] + 1} iterations, "
                    f"5-neighbour label share {share:.4f}" + ("" if png else " (no matplotlib: no picture)"))
        report["levels"].append({"level": lvl, "module": mod, "D": int(f.shape[1]), "kl_divergence": res["kl_divergence"],
                                 "n_iter": res["n_iter"], "neighbour_label_share": share, "picture": bool(png),
                                 "history": [list(h) for h in res["history"]]})
    with open(osp.join(out_dir, "tsne.json"), "w") as fh:
        json.dump(report, fh, indent=1)
    logger.info(f"wrote {osp.join(out_dir, 'tsne.json')}")
    return report


def tsne_pipeline(root_path, argv=None):
    from basicsr import knn as knn_cmd   # the probe's own reader and encoder

    args = parse_args(argv)
    logger = get_root_logger(logger_name="basicsr", log_level=logging.INFO)
    device = torch.device("cuda" if torch.cuda.is_available() else "cpu")   # (on the CPU the embedding raises: there is no fallback)
    if args.features is not None:
        feats, labels = knn_cmd.load_features(args.features)
        name, topt = osp.basename(osp.normpath(args.features)), {}
        features = [torch.from_numpy(np.ascontiguousarray(f, dtype=np.float32)).to(device) for f in feats]
        names = [f"lr_features_{i + 1}" for i in range(len(feats))]
    else:
        from basicsr.utils.misc import set_random_seed
        from basicsr.utils.options import apply_force_yml, yaml_load

        opt = apply_force_yml(yaml_load(args.opt), args.force_yml)
        set_random_seed(int(opt.get("manual_seed", 0)))
        name, topt = opt["name"], opt.get("tsne") or {}
        features, names, labels = knn_cmd.encode(opt, logger, device)
    topt = dict(topt, **{k: v for k, v in (("perplexity", args.perplexity), ("max_iter", args.max_iter)) if v is not None})
    return run(features, names, labels, topt, args.out or osp.join(root_path, "results", name), logger, name)


if __name__ == "__main__":
    tsne_pipeline(osp.abspath(osp.join(__file__, osp.pardir, osp.pardir)))
