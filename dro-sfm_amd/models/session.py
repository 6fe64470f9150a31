"""InferenceSession: the eval-mode forward of an SfmModelMF family model,
captured once per input shape into a hipGraph and replayed.

The eval forward is launch bound: about a thousand small
launches, each paid through Python dispatch when the model is called eagerly.
The training step avoids that through trainers.dp_trainer.GraphedTrainStep;
this is the same for inference.  A session stands wherever the inference
functions take a model (models.infer.infer_sequence,
models.reconstruct.reconstruct_sequence / predict_interior_frames,
models.evaluate.evaluate_depth, DataParallelTrainer.validate(session=...)):
they only use model.modules(), model.eval() and model(batch).

    session = InferenceSession(model)
    out = reconstruct_sequence(session, frames, K)

With fused_eval_bn (default) the encoders' eval-mode BatchNorm sites run as
hip.batchnorm_eval_act (networks.optim.extractor.set_fused_eval_batchnorm):
the session switches it on around its forwards and restores the previous
setting afterwards.
"""
import contextlib

import torch
import torch.nn as nn

from ..networks.optim.extractor import fused_eval_batchnorm


def _clone_tree(out):
    """Copies of every tensor of a model output (dicts, lists, tuples, tensors
    and objects with a clone() of their own: geometry.pose.Pose)."""
    if torch.is_tensor(out):
        return out.clone()
    if isinstance(out, dict):
        return type(out)((k, _clone_tree(v)) for k, v in out.items())
    if type(out) in (list, tuple):
        return type(out)(_clone_tree(v) for v in out)
    if hasattr(out, "clone"):
        return out.clone()
    return out


class _Captured:
    def __init__(self, graph, static, out, addresses):
        self.graph, self.static, self.out, self.addresses = graph, static, out, addresses


class InferenceSession(nn.Module):
    """`session(batch)` returns what `model(batch)` returns in eval mode,
    {"inv_depths": [inv], "poses": [Pose, ...]}, under no_grad; it reads
    batch["rgb"] [B,3,H,W], batch["rgb_context"] (N tensors like rgb) and
    batch["intrinsics"] [B,3,3] (float32 frames, a floating-point K, all on one
    device: anything else is refused), and refuses to run while the model is in
    training mode.

    On a CUDA device with graph=True the first call with a signature
    (B, N, H, W, device) clones the batch into static buffers, runs `warmup`
    eager forwards on a side stream (they create the forward's own side
    streams, which must exist before a capture) and captures model(static)
    into a torch.cuda.CUDAGraph in a memory pool private to the session.
    Every call with that signature copies its inputs into the static buffers,
    replays the graph on the current stream and returns COPIES of the outputs:
    a result stays valid after the next call.  At most `max_graphs` graphs are
    kept; a further signature runs eagerly (no graph is evicted).  release()
    drops the graphs and their pool.  `captures` counts the captures made.

    A graph holds addresses, not values.  In-place updates of parameters and
    buffers -- Adam over the trainer's flat buffers, load_state_dict, BatchNorm
    statistics moved by training -- are therefore seen by the next replay:
    nothing is folded or cached at capture (hip.batchnorm_eval_act reads the
    running statistics on every launch).  A parameter or buffer whose STORAGE
    was replaced (p.data = ..., model.to(...)) is found before each replay by
    comparing every data_ptr with the ones recorded at capture; that signature
    is then captured again.

    What is frozen into a graph: the module-level switches read while it was
    captured (networks.optim.extractor.set_native_convs / set_native_strided_convs
    / set_native_maxpool / set_fused_eval_batchnorm, DepthPoseNet's
    set_concurrent_blocks / set_cnet_depth_stream, DRO_BN_FUSION, ...), the
    model's hyper-parameters (version, min/max depth) and its module structure.
    Call release() after changing any of them.

    On a CPU device, or with graph=False, the session is an eager pass-through
    (the fused BN applies only where the tensors are on the GPU)."""

    def __init__(self, model, graph=True, fused_eval_bn=True, max_graphs=4, warmup=2):
        super().__init__()
        self.model = model
        self.graph, self.fused_eval_bn = bool(graph), bool(fused_eval_bn)
        self.max_graphs, self.warmup = int(max_graphs), int(warmup)
        self.captures = 0
        self._graphs = {}
        self._pool = None

    def release(self):
        """Drop every captured graph and the session's memory pool; the next
        call of a signature captures afresh."""
        self._graphs.clear()
        self._pool = None

    def _switch(self):
        return fused_eval_batchnorm(True) if self.fused_eval_bn else contextlib.nullcontext()

    def _addresses(self):
        return tuple(t.data_ptr() for t in self.model.parameters()) + tuple(t.data_ptr() for t in self.model.buffers())

    def forward(self, batch):
        if self.model.training:
            raise RuntimeError("InferenceSession: the model is in training mode; call eval() first "
                               "(the session runs the eval-mode forward only)")
        rgb, ctx, K = batch["rgb"], list(batch["rgb_context"]), batch["intrinsics"]
        for name, t in (("rgb", rgb), *((f"rgb_context[{j}]", c) for j, c in enumerate(ctx)), ("intrinsics", K)):
            if t.device != rgb.device or not t.is_floating_point() or (t is not K and t.dtype != torch.float32):
                raise RuntimeError(f"InferenceSession: batch['{name}'] is {t.dtype} on {t.device}; the frames must be "
                                   f"float32 and the whole batch on one device ({rgb.device})")
            if t is not K and t.shape != rgb.shape:
                raise RuntimeError(f"InferenceSession: batch['{name}'] {tuple(t.shape)} does not match rgb "
                                   f"{tuple(rgb.shape)}")
        with torch.no_grad(), self._switch():
            if not (self.graph and rgb.is_cuda):
                return self.model(batch)
            sig = (rgb.shape[0], len(ctx), rgb.shape[2], rgb.shape[3], rgb.device)
            cap = self._graphs.get(sig)
            if cap is not None and cap.addresses != self._addresses():
                del self._graphs[sig], cap          # a tensor of the model was replaced: capture again
                cap = None
            if cap is None:
                if len(self._graphs) >= self.max_graphs:
                    return self.model(batch)
                cap = self._graphs[sig] = self._capture(rgb, ctx, K)
            else:
                cap.static["rgb"].copy_(rgb, non_blocking=True)
                for d, s in zip(cap.static["rgb_context"], ctx):
                    d.copy_(s, non_blocking=True)
                cap.static["intrinsics"].copy_(K, non_blocking=True)
            cap.graph.replay()
            return _clone_tree(cap.out)

    def _capture(self, rgb, ctx, K):
        """GraphedTrainStep._capture_all's recipe for the eval forward: warm-up
        on a side stream (the forward's persistent side streams are created
        there, never during a capture), then a thread-local capture into the
        session's pool.  The forward forks to its side streams from the
        capturing stream and joins them before it returns, so they are part of
        the capture."""
        dev = rgb.device
        static = {"rgb": rgb.detach().clone(memory_format=torch.contiguous_format),
                  "rgb_context": [t.detach().clone(memory_format=torch.contiguous_format) for t in ctx],
                  "intrinsics": K.detach().clone(memory_format=torch.contiguous_format)}
        cur = torch.cuda.current_stream(dev)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            for _ in range(max(1, self.warmup)):
                self.model(static)
        cur.wait_stream(side)
        torch.cuda.synchronize(dev)
        if self._pool is None:
            self._pool = torch.cuda.graph_pool_handle()
        with torch.cuda.device(dev):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=self._pool, capture_error_mode="thread_local"):
                out = self.model(static)
        torch.cuda.synchronize(dev)
        self.captures += 1
        return _Captured(g, static, out, self._addresses())
