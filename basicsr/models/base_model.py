"""Caller-side base class of the hot path (reference basicsr/models/base_model.py): device placement and
the DDP wrap (:100-118), optimizer factory (:120-139), EMA (:86-95), checkpoint IO with the reference's
key conventions (:249-369), loss reduction to rank 0 (:432-457)."""
from __future__ import annotations

import os
import time
from collections import OrderedDict
from copy import deepcopy

import torch
from torch.nn.parallel import DataParallel, DistributedDataParallel

from basicsr.utils import get_root_logger
from dcpt_amd import functional as DF
from basicsr.utils.dist_util import master_only


class _PendingLog(OrderedDict):
    """losses of a step as device tensors, on their way into ``BaseModel.log_dict`` (reduce_loss_dict)"""


class BaseModel:
    def __init__(self, opt):
        self.opt = opt
        self.device = torch.device("cuda" if opt["num_gpu"] != 0 else "cpu")
        self.is_train = opt["is_train"]
        self.schedulers = []
        self.optimizers = []
        self.log_dict = OrderedDict()

    # -- protocol ---------------------------------------------------------------------------
    def feed_data(self, data):
        pass

    def _lq_on_device(self, data):
        """the degraded batch of ``feed_data``: ``data["lq"]`` moved to the device, as ever; a batch of a ``jpeg_backend: device`` set
        (PairedImageJPEGCARDataset: ``gt`` and ``jpeg_quality``, no ``lq``) gets it from the JPEG round trip of ``gt`` on the device, a
        batch of a ``demosaic_backend: device`` set (PairedImageMosaicDataset: ``gt`` and ``mosaic``, the method's index) from the demosaic
        kernel, and a batch of an ``inpaint_backend: device`` set (PairedImageInpaintingDataset: ``gt``, ``inpaint_lines``,
        ``inpaint_meta``) from the line-mask kernel, and a batch of a ``noise_backend: device`` set (PairedImageDenoiseDataset: ``gt``,
        ``noise_sigma``, ``noise_key``) from the Philox noise kernel, unclipped like the host path, and a batch of a ``blur_backend: device``
        set (PairedImageBlurDataset: ``gt`` and ``blur_kernel``, one (K, K) kernel per image) from the blur kernel, and a batch of a
        ``noise_type: poisson`` set (PairedImageDenoiseDataset: ``gt``, ``poisson_scale``, ``poisson_gray``, ``noise_key``) from the Poisson
        noise kernels, clipped as ``add_poisson_noise_pt`` defaults (single-kind batches only), and a batch of a RealESRGANDataset
        (``gt``, ``kernel1``, ``kernel2``, ``sinc_kernel``) from the second-order chain (``_lq_second_order``; single-kind batches only).  A mixed batch
        (``basicsr.data.degrade_collate``: ``degrade_kind`` per sample, each kind's keys stacked over its own samples) gets every kind's rows
        from that kind's op on its ``gt`` rows"""
        if "degrade_kind" in data:
            return self._lq_mixed(data)
        if "lq" not in data and "noise_sigma" in data:
            gt = data["gt"].to(self.device, non_blocking=True)
            return DF.gaussian_noise(gt, data["noise_sigma"], data["noise_key"])
        if "lq" not in data and "poisson_scale" in data:
            gt = data["gt"].to(self.device, non_blocking=True)
            return DF.poisson_noise(gt, data["poisson_scale"], data["noise_key"], gray=data["poisson_gray"], clip=True)
        if "lq" not in data and "jpeg_quality" in data:
            gt = data["gt"].to(self.device, non_blocking=True)
            return DF.diffjpeg(gt, data["jpeg_quality"].to(self.device, non_blocking=True), uint8_io=True)
        if "lq" not in data and "mosaic" in data:
            gt = data["gt"].to(self.device, non_blocking=True)
            methods = set(data["mosaic"].reshape(-1).tolist())   # (a host tensor: one data set, one method)
            if len(methods) != 1 or not methods <= set(range(len(DF.DEMOSAIC_METHODS))):
                raise ValueError(f"a batch carries one demosaic method, 0 (malvar) or 1 (bilinear); got {sorted(methods)}")
            return DF.demosaic(gt, DF.DEMOSAIC_METHODS[methods.pop()], uint8_io=True)
        if "lq" not in data and "inpaint_meta" in data:
            gt = data["gt"].to(self.device, non_blocking=True)
            return DF.inpaint_lines(gt, data["inpaint_lines"], data["inpaint_meta"])
        if "lq" not in data and "blur_kernel" in data:
            gt = data["gt"].to(self.device, non_blocking=True)
            return DF.filter2d(gt, data["blur_kernel"])
        if "lq" not in data and "kernel1" in data:
            return self._lq_second_order(data)
        return data["lq"].to(self.device, non_blocking=True)

    def _lq_second_order(self, data):
        """``lq`` of a RealESRGANDataset batch (``gt``, ``kernel1``, ``kernel2``, ``sinc_kernel``, no ``lq``): the second-order degradation
        chain of ``basicsr.data.degradations`` on the device, its draws made on the host from the options' top-level ``degradation:`` block
        and ``scale``.  With ``degradation.gt_usm: true`` the ground truth is ``USMSharp()(gt)``; the chain starts from it and
        ``_gt_on_device`` hands it to ``feed_data``."""
        from basicsr.data.degradations import apply_second_order, draw_second_order_plan
        from basicsr.utils import USMSharp

        opt = self.opt.get("degradation")
        if opt is None:
            raise ValueError("a batch of RealESRGANDataset needs the options' `degradation:` block (the second-order chain's ranges)")
        gt = data["gt"].to(self.device, non_blocking=True)
        if opt.get("gt_usm", False):
            if getattr(self, "_usm_sharpener", None) is None:
                self._usm_sharpener = USMSharp().to(self.device)
            with torch.no_grad():
                gt = self._usm_sharpener(gt)
        self._second_order_gt = gt
        B, _, H, W = gt.shape
        plan = draw_second_order_plan(opt, B, H, W, int(self.opt["scale"]))
        return apply_second_order(gt, data["kernel1"], data["kernel2"], data["sinc_kernel"], plan)

    def _gt_on_device(self, data):
        """``data["gt"]`` on the device; for a batch of the second-order chain the ground truth the chain started from (sharpened under
        ``gt_usm``).  Call it after ``_lq_on_device``."""
        if "lq" not in data and "kernel1" in data:
            return self._second_order_gt
        return data["gt"].to(self.device, non_blocking=True)

    def _lq_mixed(self, data):
        """``lq`` of a mixed batch: allocated like ``gt``; for each kind present the rows of that kind (read from the HOST tensor
        ``degrade_kind``: no synchronisation) are gathered from ``gt``, degraded by the kind's op and scattered back.  Demosaic rows are
        grouped by method, so one batch may hold both."""
        gt = data["gt"].to(self.device, non_blocking=True)
        kind = data["degrade_kind"].reshape(-1).tolist()
        if len(kind) != gt.shape[0] or not set(kind) <= set(range(6)):
            raise ValueError(f"degrade_kind must hold one of 0..5 for each of the {gt.shape[0]} images, got {kind}")
        lq = torch.empty_like(gt)

        def put(rows, op):
            index = torch.tensor(rows, dtype=torch.long).to(self.device, non_blocking=True)
            lq.index_copy_(0, index, op(gt.index_select(0, index)))

        for k in sorted(set(kind)):
            rows = [i for i, v in enumerate(kind) if v == k]
            if k == 0:
                put(rows, lambda g: data["lq"].to(self.device, non_blocking=True))
            elif k == 1:
                put(rows, lambda g: DF.gaussian_noise(g, data["noise_sigma"], data["noise_key"]))
            elif k == 2:
                put(rows, lambda g: DF.diffjpeg(g, data["jpeg_quality"].to(self.device, non_blocking=True), uint8_io=True))
            elif k == 3:
                methods = data["mosaic"].reshape(-1).tolist()
                if len(methods) != len(rows) or not set(methods) <= set(range(len(DF.DEMOSAIC_METHODS))):
                    raise ValueError(f"mosaic holds 0 (malvar) or 1 (bilinear) for each demosaic image; got {methods}")
                for m in sorted(set(methods)):
                    put([r for r, v in zip(rows, methods) if v == m], lambda g, m=m: DF.demosaic(g, DF.DEMOSAIC_METHODS[m], uint8_io=True))
            elif k == 4:
                put(rows, lambda g: DF.inpaint_lines(g, data["inpaint_lines"], data["inpaint_meta"]))
            else:
                put(rows, lambda g: DF.filter2d(g, data["blur_kernel"]))
        return lq

    def optimize_parameters(self, current_iter):
        pass

    def get_current_visuals(self):
        pass

    def save(self, epoch, current_iter):
        pass

    def validation(self, dataloader, current_iter, tb_logger, save_img=False, clamp=True):
        if self.opt["dist"]:
            return self.dist_validation(dataloader, current_iter, tb_logger, save_img, clamp)
        return self.nondist_validation(dataloader, current_iter, tb_logger, save_img, clamp)

    def get_current_log(self):
        return self.log_dict

    # ``log_dict`` (reference base_model.py:448-457: an OrderedDict of Python floats, filled by every optimize_parameters) is materialised
    # LAZILY: a step stores its (reduced) loss tensors and the floats are made when somebody reads the log.  The reference's ``.item()`` per
    # loss per step is a host synchronisation at the end of every step -- the device then idles until the host has launched the next step's
    # first kernels (two gaps of 3.0 + 1.4 ms per all-bf16 DCPT step on MI355X, 4 % of it; profiles/r6/dcpt_allbf16_256_kernels_sync.txt);
    # a training loop reads the log every ``print_freq`` iterations, and only those iterations synchronise.  Same values, same type.
    @property
    def log_dict(self):
        pending = self.__dict__.get("_log_pending")
        if pending is not None:
            self.__dict__["_log_pending"] = None
            keys = list(pending.keys())
            vals = [pending[k] for k in keys]
            if vals and all(torch.is_tensor(v) for v in vals) and len({v.device for v in vals}) == 1:
                # one transfer, one synchronisation (as float64: exact for an fp32 loss, and a float64 loss -- SSIMLoss -- keeps its digits)
                floats = torch.stack([v.detach().double().reshape(()) for v in vals]).tolist()
            else:
                floats = [float(v) for v in vals]
            self.__dict__["_log_values"] = OrderedDict(zip(keys, floats))
        return self.__dict__.setdefault("_log_values", OrderedDict())

    @log_dict.setter
    def log_dict(self, value):
        if isinstance(value, _PendingLog):
            self.__dict__["_log_pending"] = value
        else:
            self.__dict__["_log_pending"] = None
            self.__dict__["_log_values"] = value

    # -- networks -----------------------------------------------------------------------------
    def model_to_device(self, net, dist=True, find_unused_parameters=None):
        """One process per GPU; gradients are averaged by DDP's bucketed all-reduce over RCCL/xGMI,
        overlapped with the remaining backward kernels (each fused block returns its gradients at once)."""
        net = net.to(self.device)
        if self.opt["dist"] and dist:
            if find_unused_parameters is None:
                find_unused_parameters = self.opt.get("find_unused_parameters", False)
            kwargs = dict(find_unused_parameters=find_unused_parameters)
            if self.device.type == "cuda":
                kwargs["device_ids"] = [torch.cuda.current_device()]
                kwargs["bucket_cap_mb"] = self.opt.get("ddp_bucket_cap_mb", 64)
                kwargs["gradient_as_bucket_view"] = True
            net = DistributedDataParallel(net, **kwargs)
            if self.device.type == "cuda":
                from dcpt_amd import ddp as dcpt_ddp

                dcpt_ddp.prepare(net)   # one divide per bucket, parameter gradients written straight into the bucket views
        elif self.opt["num_gpu"] > 1 and dist:
            net = DataParallel(net)
        return net

    def get_bare_model(self, net):
        return net.module if isinstance(net, (DataParallel, DistributedDataParallel)) else net

    def get_optimizer(self, optim_type, params, lr, **kwargs):
        table = {"Adam": torch.optim.Adam, "AdamW": torch.optim.AdamW, "Adamax": torch.optim.Adamax,
                 "SGD": torch.optim.SGD, "ASGD": torch.optim.ASGD, "RMSprop": torch.optim.RMSprop,
                 "Rprop": torch.optim.Rprop}
        if optim_type not in table:
            raise NotImplementedError(f"optimizer {optim_type} is not supported yet.")
        if optim_type == "AdamW" and kwargs.get("fused") and not kwargs.get("amsgrad"):
            # ``fused: true`` asks for a fused implementation: on fp32 CUDA parameters that is the library's multi-tensor kernel
            # (dcpt_amd/optim.py: torch's update rule and state-dict layout, a handful of launches for the 664 tensors of NAFNet-64)
            params = list(params)
            flat = [p for g in params for p in g["params"]] if params and isinstance(params[0], dict) else params
            if flat and all(p.is_cuda and p.dtype == torch.float32 for p in flat):
                from dcpt_amd.optim import FusedAdamW

                return FusedAdamW(params, lr, **kwargs)
        return table[optim_type](params, lr, **kwargs)

    def setup_schedulers(self):
        """reference :141-158: MultiStepLR / MultiStepRestartLR / CosineAnnealingRestartLR by name"""
        from . import lr_scheduler as lrs

        sched = dict(self.opt["train"]["scheduler"])
        kind = sched.pop("type")
        for optimizer in self.optimizers:
            if kind in ("MultiStepLR", "MultiStepRestartLR"):
                self.schedulers.append(lrs.MultiStepRestartLR(optimizer, **sched))
            elif kind == "CosineAnnealingRestartLR":
                self.schedulers.append(lrs.CosineAnnealingRestartLR(optimizer, **sched))
            else:
                raise NotImplementedError(f"Scheduler {kind} is not implemented yet.")

    def update_learning_rate(self, current_iter, warmup_iter=-1):
        if current_iter > 1:
            for scheduler in self.schedulers:
                scheduler.step()
        if current_iter < warmup_iter:
            for optimizer in self.optimizers:
                for group in optimizer.param_groups:
                    group["lr"] = group["initial_lr"] / warmup_iter * current_iter

    def get_current_learning_rate(self):
        return [g["lr"] for g in self.optimizers[0].param_groups]

    # -- training state (reference :371-430) -------------------------------------------------------
    @master_only
    def save_training_state(self, epoch, current_iter):
        if current_iter == -1:
            return
        state = {"epoch": epoch, "iter": current_iter, "optimizers": [o.state_dict() for o in self.optimizers],
                 "schedulers": [s.state_dict() for s in self.schedulers]}
        path = os.path.join(self.opt["path"]["training_states"], f"{current_iter}.state")
        logger = get_root_logger()
        for attempt in range(3):
            try:
                torch.save(state, path)
                return
            except Exception as e:  # noqa: BLE001
                logger.warning(f"Save training state error: {e}, remaining retry times: {2 - attempt}")
                time.sleep(1)
        logger.warning(f"Still cannot save {path}. Just ignore it.")

    def resume_training(self, resume_state):
        opts, scheds = resume_state["optimizers"], resume_state["schedulers"]
        assert len(opts) == len(self.optimizers), "Wrong lengths of optimizers"
        assert len(scheds) == len(self.schedulers), "Wrong lengths of schedulers"
        for o, sd in zip(self.optimizers, opts):
            o.load_state_dict(sd)
        for s, sd in zip(self.schedulers, scheds):
            s.load_state_dict(sd)

    def model_ema(self, decay=0.999):
        src = dict(self.get_bare_model(self.net_g).named_parameters())
        dst = dict(self.net_g_ema.named_parameters())
        keys = list(dst.keys())
        with torch.no_grad():  # one multi-tensor launch pair instead of the reference's 664 mul_/add_ pairs
            torch._foreach_mul_([dst[k] for k in keys], decay)
            torch._foreach_add_([dst[k] for k in keys], [src[k].detach() for k in keys], alpha=1 - decay)
        # foreach / fused updates do not reliably bump the parameters' version counters: tell the kernels' weight caches
        # (dcpt_amd.functional.PackedWeightsBf16) explicitly that net_g_ema's parameters have new values
        DF.invalidate_packed_weights()

    # -- checkpoints ------------------------------------------------------------------------------
    @master_only
    def save_network(self, net, net_label, current_iter, param_key="params"):
        name = "latest" if current_iter == -1 else current_iter
        path = os.path.join(self.opt["path"]["models"], f"{net_label}_{name}.pth")
        nets = net if isinstance(net, list) else [net]
        keys = param_key if isinstance(param_key, list) else [param_key]
        assert len(nets) == len(keys), "The lengths of net and param_key should be the same."
        payload = {}
        for n, k in zip(nets, keys):
            sd = self.get_bare_model(n).state_dict()
            payload[k] = OrderedDict((kk[7:] if kk.startswith("module.") else kk, v.cpu()) for kk, v in sd.items())
        logger = get_root_logger()
        for attempt in range(3):
            try:
                torch.save(payload, path)
                return
            except Exception as e:  # noqa: BLE001
                logger.warning(f"Save model error: {e}, remaining retry times: {2 - attempt}")
                time.sleep(1)
        logger.warning(f"Still cannot save {path}. Just ignore it.")

    def _print_different_keys_loading(self, crt_net, load_net, strict=True):
        crt = self.get_bare_model(crt_net).state_dict()
        a, b = set(crt.keys()), set(load_net.keys())
        logger = get_root_logger()
        if a != b:
            logger.warning("Current net - loaded net:")
            for v in sorted(a - b):
                logger.warning(f"  {v}")
            logger.warning("Loaded net - current net:")
            for v in sorted(b - a):
                logger.warning(f"  {v}")
        if not strict:
            for k in a & b:
                if crt[k].size() != load_net[k].size():
                    logger.warning(f"Size different, ignore [{k}]: crt_net: {crt[k].shape}; load_net: {load_net[k].shape}")
                    load_net[k + ".ignore"] = load_net.pop(k)

    def load_network(self, net, load_path, strict=True, param_key="params", remove_norm=False):
        logger = get_root_logger()
        net = self.get_bare_model(net)
        load_net = torch.load(load_path, map_location="cpu")
        if param_key is not None:
            if param_key not in load_net and "params" in load_net:
                param_key = "params"
                logger.info("Loading: params_ema does not exist, use params.")
            load_net = load_net[param_key]
        logger.info(f"Loading {net.__class__.__name__} model from {load_path}, with param key: [{param_key}].")
        for k, v in deepcopy(load_net).items():
            if "norm" in k and remove_norm:
                continue
            if k.startswith("module."):
                load_net[k[7:]] = v
                load_net.pop(k)
        self._print_different_keys_loading(net, load_net, strict)
        net.load_state_dict(load_net, strict=strict)
        DF.invalidate_packed_weights()

    # -- logging ----------------------------------------------------------------------------------
    def reduce_loss_dict(self, loss_dict):
        with torch.no_grad():
            if self.opt["dist"]:
                keys = list(loss_dict.keys())
                losses = torch.stack([loss_dict[k] for k in keys], 0)
                torch.distributed.reduce(losses, dst=0)
                if self.opt["rank"] == 0:
                    losses /= self.opt["world_size"]
                loss_dict = {k: v for k, v in zip(keys, losses)}
            # (0-d device tensors, not floats: ``log_dict`` turns them into floats when the log is read -- no synchronisation in the step)
            return _PendingLog((k, v.detach().mean()) for k, v in loss_dict.items())
