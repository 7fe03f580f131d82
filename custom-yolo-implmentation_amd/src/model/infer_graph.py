"""Replayed inference: forward + decode of `Model.inference` (reference src/model/model_builder.py:115-139) as one hipGraph
per input shape.

A single 640 x 640 image is ~220 launches of 2 - 30 us: issued one by one the host is the bottleneck (preset s: 2.7 ms per
image eager against 0.94 ms replayed, preset l: 4.5 against 1.9 -- tools/infer_bench.py).  The graph holds the static input,
every intermediate, the decoded (N, 4 + nc, M) tensor and the class-aware NMS on it (its launches have fixed grids: the
candidate capacity, not the candidate count) in its own pool; a call copies the image in, replays, reads the per-image
counts (the one device -> host sync of non_max_suppression) and returns CLONED rows, so nothing a caller keeps aliases the pool.

Validity: the unfused model's kernels read parameters and BatchNorm buffers where they live, so in-place updates
(optimizer steps, load_state_dict) are seen by the next replay.  What a replay cannot follow is a change of STORAGE or of the
module tree: `Model._apply` (.to / .half / .cuda), `fuse()` and `load_weights()` drop the graphs, and so does any change of
the parameters' version counters (a fused conv keeps a packed copy of its frozen weight inside the graph).

`Model.predict` (no reference counterpart) keeps its entries here too, keyed by slot count, canvas size, source capacity, dtype,
autocast state and the NMS arguments: the graph runs letterbox -> forward -> decode -> NMS -> rows_to_source on a static uint8 source
buffer (a power of two of bytes, so pictures of other sizes replay the same graph) and a static record table; a call copies the
packed pictures and the table in, replays and reads the counts."""
import collections
import warnings

import torch

from src.hipops import ops


class InferenceGraphs:
    MAX_SHAPES = 4                        # distinct (shape, dtype, autocast) keys kept; the least recently used one goes first
    MIN_SOURCE_BYTES = 1 << 20            # floor of a predict entry's source capacity (a 640 x 480 picture is 0.9 MB)

    def __init__(self):
        self.entries = collections.OrderedDict()
        self.disabled = None              # reason, once a capture has failed: that model runs eagerly from then on
        self.tensors = None
        self.modules = None

    def _stamp(self, model):
        """Sum of the version counters of every parameter and buffer (walking the module tree costs ~0.8 ms on preset s, so
        the tensor list is kept; whatever replaces tensors or modules -- _apply, fuse, load_weights -- drops this object)."""
        if self.tensors is None:
            self.tensors = list(model.parameters()) + list(model.buffers())
        return sum(t._version for t in self.tensors)

    def all_eval(self, model):
        """Whether every module is in eval mode already -- what `model.eval()` would establish, without its walk over the
        module tree on every call (~0.8 ms on preset s; the module list is kept like the tensor list)."""
        if self.modules is None:
            self.modules = list(model.modules())
        return not any(m.training for m in self.modules)

    def _entry(self, model, key, capture):
        """The captured entry of `key`, made by `capture()` when there is none or the weights have changed since; None = the
        capture failed, and this model runs launch by launch from then on."""
        stamp = self._stamp(model)
        ent = self.entries.get(key)
        if ent is not None and ent["stamp"] != stamp:
            ent = None
            self.entries.clear()                              # weights changed: every graph may hold stale packed copies
        if ent is None:
            try:
                ent = capture()
            except Exception as e:                            # noqa: BLE001 -- a model that cannot be captured stays usable
                self.disabled = f"{type(e).__name__}: {e}"
                warnings.warn(f"inference graph capture failed ({self.disabled}); running eagerly", stacklevel=4)
                return None
            ent["stamp"] = self._stamp(model)                 # (a first eval pass may touch buffers' counters)
            self.entries[key] = ent
            while len(self.entries) > self.MAX_SHAPES:
                self.entries.popitem(last=False)
        self.entries.move_to_end(key)
        return ent

    def run(self, model, image, conf_thres, iou_thres):
        """Detections (list of (n, 6) tensors, as non_max_suppression returns them) for `image` (a device tensor), replayed;
        None = run eagerly."""
        if self.disabled is not None or not image.is_cuda or model.training or torch.is_grad_enabled():
            return None
        amp = torch.is_autocast_enabled()
        if not (0 <= conf_thres <= 1 and 0 <= iou_thres <= 1):
            return None                                       # non_max_suppression raises the reference's assertion
        key = (tuple(image.shape), image.dtype, image.device.index, amp, torch.get_autocast_dtype("cuda") if amp else None,
               float(conf_thres), float(iou_thres))
        ent = self._entry(model, key, lambda: self._capture(model, image, amp, float(conf_thres), float(iou_thres)))
        if ent is None:
            return None
        ent["x"].copy_(image)
        ent["graph"].replay()
        rows, counts, status = ent["y"]
        host = torch.cat((counts, status)).tolist()           # the one device -> host sync, as in non_max_suppression
        if host[-1]:
            raise RuntimeError("yolo_nms: more candidates than the kernel capacity; raise conf_thres")
        rows = rows.clone()
        return [rows[i, :host[i]] for i in range(image.shape[0])]

    def run_predict(self, model, pinned, nbytes, table_host, size, dtype, logit_thres, iou, max_det, agnostic, classes):
        """`Model.predict`'s chunk, replayed: the packed uint8 sources `pinned[:nbytes]` and their pinned letterbox table go
        into the entry's static buffers, one replay runs letterbox -> forward -> decode -> NMS -> rows_to_source, and the one
        host sync reads the counts.  -> (cloned rows fp32 [slots][max_det][6], counts), or None = run launch by launch."""
        if self.disabled is not None or model.training or torch.is_grad_enabled():
            return None
        amp = torch.is_autocast_enabled()
        device = next(model.parameters()).device
        cap = max(self.MIN_SOURCE_BYTES, 1 << max(0, int(nbytes) - 1).bit_length())    # next power of two at or above the bytes
        key = ("predict", table_host.numel(), int(size), cap, dtype, device.index, amp, torch.get_autocast_dtype("cuda") if amp else None,
               float(logit_thres), float(iou), int(max_det), bool(agnostic), classes)
        ent = self._entry(model, key, lambda: self._capture_predict(model, device, cap, pinned, nbytes, table_host, size, dtype, amp,
                                                                    logit_thres, iou, max_det, agnostic, classes))
        if ent is None:
            return None
        ent["src"][:nbytes].copy_(pinned[:nbytes], non_blocking=True)
        ent["table"].copy_(table_host, non_blocking=True)
        ent["graph"].replay()
        rows, counts, status = ent["y"]
        host = torch.cat((counts, status)).tolist()           # the one device -> host sync; the uploads have left the pinned buffers
        if host[-1]:
            raise RuntimeError("yolo_nms: more candidates than the kernel capacity; raise conf")
        return rows.clone(), host[:-1]

    @staticmethod
    def predict_launches(model, src, table, size, dtype, logit_thres, iou, max_det, agnostic, classes):
        """The launch sequence of a predict chunk -- what the graph captures and what the launch-by-launch path issues:
        -> (rows, counts, status) on the device, rows in each source image's own pixels with probabilities as scores."""
        from src.data.letterbox import FILL
        from src.data.transforms import MEAN, STD
        x = ops.letterbox(src, table, size, FILL, dtype, MEAN, STD)
        preds, anchors, strides = model.forward(x)
        y = ops.head_decode(preds, anchors, strides, model.head.nc)
        rows, counts, status = ops.nms(y, model.num_classes, logit_thres, iou, classes, agnostic, False, max_det)
        ops.rows_to_source(rows, counts, table, True)
        return rows, counts, status

    @classmethod
    def _capture_predict(cls, model, device, cap, pinned, nbytes, table_host, size, dtype, amp, logit_thres, iou, max_det, agnostic,
                         classes):
        src = torch.zeros(cap, dtype=torch.uint8, device=device)
        src[:nbytes].copy_(pinned[:nbytes])                    # the warm-up passes run on real pictures and a checked table
        table = table_host.to(device)
        ent = cls._capture_fn(lambda: cls.predict_launches(model, src, table, size, dtype, logit_thres, iou, max_det, agnostic, classes),
                              device, amp)
        ent.update(src=src, table=table)
        return ent

    @classmethod
    def _capture(cls, model, image, amp, conf_thres, iou_thres):
        nc = model.head.nc
        x = image.clone()

        def fwd():
            preds, anchors, strides = model.forward(x)
            y = ops.head_decode(preds, anchors, strides, nc)
            return ops.nms(y, model.num_classes, conf_thres, iou_thres, None, False, False, 300)

        ent = cls._capture_fn(fwd, image.device, amp)
        ent["x"] = x
        return ent

    @staticmethod
    def _capture_fn(fwd, device, amp):
        cur = torch.cuda.current_stream(device)
        side = torch.cuda.Stream(device)
        side.wait_stream(cur)
        with torch.cuda.stream(side):                         # warm-up off the capture: packed weights, anchors, allocator
            for _ in range(2):
                fwd()
        cur.wait_stream(side)
        torch.cuda.synchronize(device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            if amp:                                           # no cast cache: a cached cast would live in the graph's pool
                with torch.autocast("cuda", dtype=torch.get_autocast_dtype("cuda"), cache_enabled=False):
                    y = fwd()
            else:
                y = fwd()
        return dict(y=y, graph=g)
