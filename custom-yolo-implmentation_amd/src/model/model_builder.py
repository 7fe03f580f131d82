"""Model = Backbone + Neck + Head with the reference's API (src/model/model_builder.py:13-139):
forward(x) -> (preds[N,64+nc,M], anchors[2,M], strides[1,M]); fuse(); load_weights(); inference()."""
import os
from typing import List

import torch
from torch import nn

from src.hipops import functions as F_
from src.hipops import ops
from src.model.backbone import Backbone
from src.model.head import Head
from src.model.infer_graph import InferenceGraphs
from src.model.model_blocks import Conv
from src.model.neck import Neck
from src.utils.model_utils import fuse_conv, non_max_suppression


NECK_DIRECT = os.environ.get("YOLO_NECK_DIRECT", "1") == "1"


class Model(nn.Module):
    # TrainStepRunner's staged backward: a callable that receives the backbone's outputs and returns what the neck should
    # read instead (detached leaves), cutting the autograd graph at the backbone / neck boundary
    stage_cut = None
    # inference() replays forward + decode as one hipGraph per input shape (src/model/infer_graph.py); False, or
    # YOLO_INFER_GRAPH=0 in the environment, issues the launches one by one as forward() does
    graph_inference = os.environ.get("YOLO_INFER_GRAPH", "1") == "1"
    # predict()'s default canvas: the square side the reference trains and infers at (its config.yaml's input_size)
    input_size = 640

    def __init__(self, width: List[int], depth: List[int], csp: List[bool], num_classes: int):
        super().__init__()
        self.net = Backbone(width, depth, csp)
        self.fpn = Neck(width, depth, csp)
        self.num_classes = num_classes
        self.head = Head(num_classes, (width[3], width[4], width[5]))
        # The reference measures the strides with a 640x640 CPU dummy pass (:37-45); they are fixed by
        # the architecture (three / four / five stride-2 stages), so no pass is needed here.
        self.head.stride = torch.tensor([8.0, 16.0, 32.0])
        self.stride = self.head.stride
        for m in self.modules():                 # BatchNorm's num_batches_tracked: one multi-tensor add per
            if type(m) is Conv:                  # forward instead of one tiny kernel per layer
                m._count_batches = False
        self._infer_graphs = None
        self._bn_convs = None
        self._predict_pinned = None              # predict()'s reused pinned upload buffer

    def _apply(self, fn, *args, **kwargs):       # .to() / .half() / .cuda(): new storages -- captured graphs point at the old
        self._infer_graphs = None
        self._bn_convs = None
        return super()._apply(fn, *args, **kwargs)

    def forward(self, x):
        if not self.training:
            # packed weights served by a training pass's plan predate the last optimizer step (a raw kernel updates the
            # parameters without touching their version counters): evaluation always packs afresh
            ops.ACTIVE_PACK_PLAN = None
            return self.head(list(self.fpn(self.net(x))))
        convs = self._bn_convs                   # (walking the module tree costs ~0.8 ms per eager step on preset s)
        if convs is None:
            convs = self._bn_convs = [m for m in self.modules() if type(m) is Conv and hasattr(m, "norm")]
        torch._foreach_add_([m.norm.num_batches_tracked for m in convs], 1)
        self._prepack(x, convs)
        # one zeroed pool for every layer's BatchNorm accumulators of this pass (a single memset)
        F_.BnArena.current = F_.BnArena(x.device, F_.BnArena.elems_for([m.conv.out_channels for m in convs]))
        try:
            # the neck's concat buffers; the backbone writes p3 / p4 / p5 into them (YOLO_NECK_DIRECT=0: A/B runs)
            bufs, outs = self.fpn.alloc(x) if NECK_DIRECT else (None, None)
            feats = self.net(x, outs)
            if self.stage_cut is not None:
                feats = self.stage_cut(feats)
            return self.head(list(self.fpn(feats, bufs)))
        finally:
            F_.BnArena.current = None

    def _prepack(self, x, convs):
        """Pack every dense conv weight (forward + dgrad forms) with one launch instead of two per layer.
        Only for plain local parameters; sharded/wrapped parameters (FSDP) fall back to per-layer packing."""
        ops.ACTIVE_PACK_PLAN = None
        if getattr(self, "prepack", None) is False:  # (True: TrainStepRunner; unset: decided per pass from the weights)
            return
        dense = [(m.conv.weight, m._k, m._s) for m in convs if not m._dw and m.conv.in_channels != 3]
        dense += [(b[-1].weight, 1, 1) for br in (self.head.box, self.head.cls) for b in br]
        # plain, resident local tensors only -- never what a sharding wrapper manages: FSDP2 holds DTensors until a group is
        # unsharded, FSDP1's original parameters are views of a flat parameter whose storage is freed between uses
        for w, _, _ in dense:
            if type(w.data) is not torch.Tensor or not w.is_cuda or w.dim() != 4 or getattr(w, "_fsdp_flattened", False) or \
                    w.untyped_storage().size() < w.numel() * w.element_size():
                return
        T = F_.compute_dtype(x, dense[0][0])
        key = (T, tuple(w.data_ptr() for w, _, _ in dense))
        plan = getattr(self, "_pack_plan", None)
        if plan is None or (plan.dtype, plan.key) != key:
            plan = self._pack_plan = ops.WeightPackPlan(dense, T)
        plan.run()
        ops.ACTIVE_PACK_PLAN = plan

    def fuse(self):
        """Fold every Conv's BatchNorm into its conv (inference only), reference :52-58."""
        self._infer_graphs = None
        self._bn_convs = None
        for m in self.modules():
            if type(m) is Conv and hasattr(m, "norm"):
                m.conv = fuse_conv(m.conv, m.norm)
                m.forward = m.fuse_forward
                delattr(m, "norm")
        return self

    def load_weights(self, weights_path):
        checkpoint = torch.load(weights_path, map_location=next(self.parameters()).device)
        state = checkpoint["model_state"] if isinstance(checkpoint, dict) and "model_state" in checkpoint else checkpoint
        # checkpoints written under DDP / FSDP1 carry wrapper prefixes ("module." ...): the reference's own load fails on
        # them (notebooks/04); keys are matched by their canonical names here
        from src.training.utils_train import canonical_state_dict
        self.load_state_dict(canonical_state_dict(state))
        self._infer_graphs = None
        print(f"Weights loaded successfully from {weights_path}")

    def inference(self, image, conf_thres=0.25, iou_thres=0.45):
        """Detections [x1,y1,x2,y2,conf,cls] per image; class scores are the raw logits, as in the
        reference (:115-139).  Decode (DFL expectation -> xywh -> *stride) is one fused kernel."""
        graphs = self._graphs()
        if isinstance(image, str):
            from PIL import Image
            image = Image.open(image).convert("RGB")
        if not isinstance(image, torch.Tensor):
            try:
                from PIL import Image
                is_pil = isinstance(image, Image.Image)
            except ImportError:
                is_pil = False
            if not is_pil:
                raise ValueError("Unsupported image type. Must be path, PIL Image, or Tensor.")
            from src.data.transforms import get_val_transforms
            image = get_val_transforms(device=next(self.parameters()).device)([image])[0]      # resize + normalise on the device
        if image.dim() == 3:
            image = image.unsqueeze(0)
        image = image.to(next(self.parameters()).device)
        with torch.no_grad():
            if graphs is not None and image.is_cuda:
                dets = graphs.run(self, image, conf_thres, iou_thres)
                if dets is not None:
                    return dets
            preds, anchors, strides = self.forward(image)
            y = ops.head_decode(preds, anchors, strides, self.head.nc)
            return non_max_suppression(y, conf_thres=conf_thres, iou_thres=iou_thres, nc=self.num_classes)

    def _graphs(self):
        """The replayed-inference state (None: graph_inference is off), with every module put into eval mode."""
        graphs = None
        if self.graph_inference:
            if self._infer_graphs is None:
                self._infer_graphs = InferenceGraphs()
            graphs = self._infer_graphs
        if graphs is None or not graphs.all_eval(self):
            self.eval()
        return graphs

    def predict(self, images, conf=0.25, iou=0.45, max_det=300, classes=None, agnostic=False, size=None, scaleup=True, batch=None):
        """Detections for pictures of any sizes, in each picture's own pixels (no reference counterpart; `inference` above keeps
        the reference's semantics).  images: one image or a list of images, each a path, a PIL image, a numpy array or a torch
        uint8 tensor (arrays and tensors HWC, RGB).  Every picture is letterboxed onto a `size` x `size` canvas (default
        `input_size`): resized by one gain to an integer size, centred, grey bars (`scaleup=False`: never enlarged).  `conf` is
        a PROBABILITY in (0, 1) -- the NMS runs on the logits at log(conf / (1 - conf)) -- and the returned score is the sigmoid
        of the class logit.  -> one (n_i, 6) fp32 tensor [x1, y1, x2, y2, confidence, class] per picture, cloned.
        `batch=k` runs the pictures in chunks of k slots (a short last chunk is padded with blank slots), so lists of any
        length replay one captured graph.  One chunk = one upload of the packed uint8 sources, one replay of letterbox ->
        forward -> decode -> NMS -> map back (src/model/infer_graph.py; launch by launch where `inference` would be), one sync."""
        import math

        from src.data.letterbox import letterbox_records
        from src.data.transforms import BatchTransform
        if not 0.0 < conf < 1.0:
            raise ValueError(f"predict: conf is a probability in (0, 1), got {conf}")
        if not 0.0 <= iou <= 1.0:
            raise ValueError(f"predict: iou lies in [0, 1], got {iou}")
        if int(max_det) < 1 or (batch is not None and int(batch) < 1):
            raise ValueError("predict: max_det and batch are at least 1")
        size = int(size) if size is not None else int(self.input_size)
        classes = tuple(int(c) for c in classes) if classes is not None else None
        if not isinstance(images, (list, tuple)):
            images = [images]
        imgs = []
        for im in images:
            if isinstance(im, str):
                from PIL import Image
                im = Image.open(im)
            try:
                imgs.append(BatchTransform._as_u8(im))
            except ValueError:
                raise ValueError("predict: an image is a path, a PIL image or a uint8 (H, W, 3) RGB array / tensor") from None
        param = next(self.parameters())
        if not param.is_cuda:
            raise RuntimeError("predict runs on the GPU: the product path has no CPU fallback")
        graphs = self._graphs()
        thres = math.log(conf / (1.0 - conf))
        slots = int(batch) if batch is not None else len(imgs)
        out = []
        with torch.no_grad():
            for lo in range(0, len(imgs), max(1, slots)):
                chunk = imgs[lo:lo + slots]
                recs, nbytes = letterbox_records([(t.shape[0], t.shape[1]) for t in chunk], size, scaleup, slots)
                if self._predict_pinned is None or self._predict_pinned.numel() < nbytes:
                    self._predict_pinned = torch.empty(max(1 << 20, int(nbytes * 1.25)), dtype=torch.uint8).pin_memory()
                pinned = self._predict_pinned               # (free again: every chunk ends in a host sync behind its upload)
                for t, r in zip(chunk, recs):
                    pinned[r[0]:r[0] + t.numel()].copy_(t.reshape(-1))
                table = ops.letter_table(recs, size, nbytes)
                args = (size, param.dtype, thres, iou, int(max_det), bool(agnostic), classes)
                res = graphs.run_predict(self, pinned, nbytes, table, *args) if graphs is not None else None
                if res is None:
                    src = pinned[:nbytes].to(param.device, non_blocking=True)
                    rows, counts, status = InferenceGraphs.predict_launches(self, src, table.to(param.device, non_blocking=True), *args)
                    host = torch.cat((counts, status)).tolist()
                    if host[-1]:
                        raise RuntimeError("yolo_nms: more candidates than the kernel capacity; raise conf")
                    res = rows, host[:-1]
                rows, counts = res
                out += [rows[i, :counts[i]] for i in range(len(chunk))]     # (a blank slot's rows are dropped)
        return out
