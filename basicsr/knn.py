"""``python basicsr/knn.py -opt <yml>``: the reference's "KNN" workflow (``python knn_gen.py`` then ``python knn.py``) as one command on the
HIP path.  It builds ``network_g``, hooks its decoder groups (``knn.hook_names`` / ``knn.hook_depth``, the rule of DCPTModel), runs the listed
test-phase data sets through it, keeps the flattened feature maps on the device and, per hook level, fits the 5-nearest-neighbour
classifier over the five seeded 67/33 splits of the reference with ``basicsr.utils.knn_probe`` (fp64 distances on the fp64 matrix cores,
the vote on the device).  It prints the per-seed tables and writes ``results/<name>/knn_report.json``.

Weights: ``path.pretrain_network_g`` when set (``param_key_g``, ``strict_load_g`` as for test.py); without it the reference's random init
under ``manual_seed`` (knn_gen.py:86-95): ``kaiming_uniform_(weight, a=2)`` and zero biases on every Conv2d and Linear.
Data: every set of ``datasets`` is built with ``build_dataset`` in the test phase (``center_crop: 128``), its ``dataset_idx`` is the label of
its images, and at most ``max_per_set`` (default 100) images are taken in SORTED file order -- the reference takes the first 100 of
``os.listdir``, whose order is the file system's; a set whose root is missing falls back to seeded synthetic pairs as everywhere else.
Each ``lq`` is reflect-padded to a multiple of ``knn.window_size`` (default 8, knn_gen.py:23-31) and the encoder runs in batches of
``knn.batch_size``.  ``knn.save_features: true`` also writes the reference's ``lr_features_{1..}.npy`` and ``lr_labels.npy`` next to the
report.

``python basicsr/knn.py --features DIR`` skips the network and probes such a directory: the reference's knn.py flow, for every
``lr_features_<i>.npy`` it holds.  The distances need the device: there is no CPU fallback."""
import argparse
import json
import logging
import os
import sys
from os import path as osp

sys.path.insert(0, osp.abspath(osp.join(osp.dirname(__file__), osp.pardir)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from basicsr.utils import FeatureTaps, get_root_logger, knn_probe  # noqa: E402
from basicsr.utils.knn_probe import KNN_SEEDS  # noqa: E402


def reference_init(net, seed):
    """knn_gen.py:86-95 under ``manual_seed``"""
    torch.manual_seed(int(seed))

    def init(m):
        if isinstance(m, (torch.nn.Conv2d, torch.nn.Linear)):
            torch.nn.init.kaiming_uniform_(m.weight, a=2)
            if m.bias is not None:
                torch.nn.init.constant_(m.bias, 0)

    net.apply(init)
    return net


def load_weights(net, path, param_key="params", strict=True):
    state = torch.load(path, map_location="cpu")
    for key in (param_key, "params"):   # (base_model.load_network: the named key, else "params", else a bare state dict)
        if key is not None and key in state:
            state = state[key]
            break
    state = {(k[7:] if k.startswith("module.") else k): v for k, v in state.items()}
    net.load_state_dict(state, strict=strict)
    return net


def pad_to_window(img, window_size=8):
    """knn_gen.py:23-31: reflect padding on the right and the bottom to a multiple of ``window_size``"""
    h, w = img.shape[-2:]
    ph, pw = (-h) % window_size, (-w) % window_size
    return torch.nn.functional.pad(img, (0, pw, 0, ph), "reflect") if ph or pw else img


def collect_images(opt, logger):
    """[(lq CHW tensor, label)] of every listed set: at most ``max_per_set`` images in sorted order, the label the set's ``dataset_idx``"""
    from basicsr.data import build_dataset

    kopt = opt.get("knn") or {}
    items = []
    for key, dataset_opt in sorted(opt["datasets"].items()):
        dataset_opt = dict(dataset_opt)
        dataset_opt["phase"] = "test"
        if "dataset_idx" not in dataset_opt:
            raise ValueError(f"datasets.{key}: dataset_idx (the degradation label of the set) is required")
        ds = build_dataset(dataset_opt)
        n = min(len(ds), int(dataset_opt.get("max_per_set", kopt.get("max_per_set", 100))))
        for i in range(n):
            sample = ds[i]
            if "lq" not in sample:
                raise ValueError(f"datasets.{key}: the samples carry no lq (a device degradation backend); the probe reads host lq images")
            items.append((sample["lq"], int(dataset_opt["dataset_idx"])))
        logger.info(f"{dataset_opt.get('name', key)}: {n} images, label {dataset_opt['dataset_idx']}")
    if not items:
        raise ValueError("no images: the option file lists no data set")
    return items


def encode(opt, logger, device):
    """the per-level feature matrices (on the device), the hooked module names and the labels"""
    from basicsr.archs import build_network

    kopt = opt.get("knn") or {}
    net = build_network(opt["network_g"])
    path = (opt.get("path") or {}).get("pretrain_network_g")
    if path:
        load_weights(net, osp.expanduser(path), opt["path"].get("param_key_g", "params"), opt["path"].get("strict_load_g", True))
        logger.info(f"loaded {path}")
    else:
        reference_init(net, opt.get("manual_seed", 0))
        logger.info(f"no pretrain_network_g: the reference's random init under manual_seed {opt.get('manual_seed', 0)}")
    net = net.to(device).eval()
    items = collect_images(opt, logger)
    window, batch = int(kopt.get("window_size", 8)), int(kopt.get("batch_size", 10))
    labels = np.array([lab for _, lab in items], dtype=np.int64)
    with FeatureTaps(net, kopt.get("hook_names", opt.get("hook_names")), kopt.get("hook_depth", opt.get("hook_depth", 1)), rows=len(items),
                     hook=True) as taps:
        for b0 in range(0, len(items), batch):
            imgs = [pad_to_window(img[None], window)[0] for img, _ in items[b0:b0 + batch]]
            if len({tuple(i.shape) for i in imgs}) != 1:
                raise ValueError(f"images of different sizes {sorted({tuple(i.shape) for i in imgs})}: give every set the same center_crop")
            taps(torch.stack(imgs).to(device))
        return taps.features, taps.names, labels


def load_features(directory):
    """the reference's dump: lr_labels.npy and lr_features_1.npy, lr_features_2.npy, ... as long as they exist"""
    labels = np.load(osp.join(directory, "lr_labels.npy")).reshape(-1).astype(np.int64)
    feats, i = [], 1
    while osp.isfile(osp.join(directory, f"lr_features_{i}.npy")):
        f = np.load(osp.join(directory, f"lr_features_{i}.npy"))
        feats.append(f.reshape(f.shape[0], -1))
        i += 1
    if not feats:
        raise FileNotFoundError(f"{directory} holds no lr_features_1.npy")
    return feats, labels


def run(features, names, labels, kopt, out_dir, logger, name):
    report = {"name": name, "n": int(len(labels)), "labels": sorted({int(v) for v in labels}), "levels": []}
    for lvl, (f, mod) in enumerate(zip(features, names), start=1):
        per_seed, mean = knn_probe(f, labels, n_neighbors=int(kopt.get("n_neighbors", 5)), test_size=float(kopt.get("test_size", 0.33)),
                                   seeds=tuple(kopt.get("seeds", KNN_SEEDS)))
        for r in per_seed:
            logger.info(f"level {lvl} ({mod}, D = {f.shape[1]}), seed {r['seed']}:\n{r['text']}")
        logger.info(f"level {lvl} ({mod}): mean accuracy over {len(per_seed)} seeds {mean:.4f}")
        report["levels"].append({"level": lvl, "module": mod, "D": int(f.shape[1]), "dtype": str(f.dtype).replace("torch.", ""),
                                 "mean_accuracy": mean,
                                 "seeds": [{"seed": r["seed"], "accuracy": r["accuracy"], "report": r["report"], "pred": r["pred"].tolist(),
                                            "test_idx": r["test_idx"].tolist()} for r in per_seed]})
    os.makedirs(out_dir, exist_ok=True)
    with open(osp.join(out_dir, "knn_report.json"), "w") as fh:
        json.dump(report, fh, indent=1)
    logger.info(f"wrote {osp.join(out_dir, 'knn_report.json')}")
    return report


def knn_pipeline(root_path, argv=None):
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("-opt", type=str, default=None, help="Path to option YAML file.")
    parser.add_argument("--features", type=str, default=None, help="probe a directory of lr_features_<i>.npy / lr_labels.npy instead")
    parser.add_argument("--out", type=str, default=None, help="output directory (default results/<name>)")
    parser.add_argument("--force_yml", nargs="+", default=None, help="e.g. knn:batch_size=4")
    args = parser.parse_args(argv)
    if (args.opt is None) == (args.features is None):
        parser.error("give either -opt FILE or --features DIR")
    logger = get_root_logger(logger_name="basicsr", log_level=logging.INFO)
    device = torch.device("cuda" if torch.cuda.is_available() else "cpu")   # (on the CPU the probe raises: there is no fallback)
    if args.features is not None:
        feats, labels = load_features(args.features)
        name = osp.basename(osp.normpath(args.features))
        kopt = {}
        features = [torch.from_numpy(np.ascontiguousarray(f, dtype=np.float32)).to(device) for f in feats]
        names = [f"lr_features_{i + 1}" for i in range(len(feats))]
    else:
        from basicsr.utils.misc import set_random_seed
        from basicsr.utils.options import apply_force_yml, yaml_load

        opt = apply_force_yml(yaml_load(args.opt), args.force_yml)
        set_random_seed(int(opt.get("manual_seed", 0)))
        name, kopt = opt["name"], opt.get("knn") or {}
        features, names, labels = encode(opt, logger, device)
    out_dir = args.out or osp.join(root_path, "results", name)
    if args.features is None and kopt.get("save_features", False):
        os.makedirs(out_dir, exist_ok=True)
        for i, f in enumerate(features, start=1):
            np.save(osp.join(out_dir, f"lr_features_{i}.npy"), f.float().cpu().numpy())
        np.save(osp.join(out_dir, "lr_labels.npy"), labels)
    return run(features, names, labels, kopt, out_dir, logger, name)


if __name__ == "__main__":
    knn_pipeline(osp.abspath(osp.join(__file__, osp.pardir, osp.pardir)))
