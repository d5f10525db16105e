"""The parameter updates of ``HipEngine`` and the error words that can withhold them: the fused SGD kernel, the planned optimizers
(csrc/optim.hip), the whole step captured into a HIP graph, and the stream-K / all-reduce error-word check behind every update.
Gradient-norm clipping (csrc/clip.hip) sits in front of every update.
A mixin: its state (``_steps``, ``_optim_kind``, ``exp_avg_sq``, ``_group_of*``, ``_clip_scratch``, ``last_grad_norm``, ``max_grad_norm``) is declared in
``HipEngine.__init__``."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib


def clip_grad_norm(engine, max_norm, grad_scale=1.0):
    """``torch.nn.utils.clip_grad_norm_`` on ``engine.grads``, on the device: two launches on the current stream, no host read
    (``OptimMixin._clip_grad_norm``).  Returns ``engine.last_grad_norm``, the 0-dim device view of the norm before clipping.  For a
    caller that takes the step apart (gradients, clip, update as separate calls); ``engine.max_grad_norm = bound`` makes every
    ``train_step`` do the same in front of its update."""
    return engine._clip_grad_norm(max_norm, grad_scale)


class OptimMixin:
    STREAMK_CHECK_EVERY = 64

    def sgd_step(self, lr, momentum=0.9, weight_decay=0.0, grad_scale=1.0, nesterov=False, _pipelined=False):
        if not _pipelined:             # a direct call while a pipelined update is still running on the second stream
            self.dp_flush()
        if self._optim_kind not in (None, "sgd"):
            raise _lib.PevitError(f"sgd_step: the optimizer state belongs to {self._optim_kind!r}; call reset_optimizer() first")
        flags = int(self._steps == 0) | (2 if nesterov else 0)
        _lib.check(self.lib.pevit_sgd_step(self._ctx, _lib.stream_ptr(), lr, momentum, weight_decay, grad_scale, flags), "pevit_sgd_step")
        self._after_update()

    def _after_update(self):
        """Behind every update (``sgd_step``, ``optimizer_step``, a graph replay), then the step is counted: the fused kernels skip
        the update on device when a stream-K hand-off of this step timed out; the host reads the error word on the first step and
        then every STREAMK_CHECK_EVERY steps (each check synchronises the stream) ... and with the flat all-reduce as the exchange
        EVERY step: a rank whose reduction gave up withholds its update while its peers apply theirs, and replicas must not drift
        apart for 64 steps before anybody notices.  (A graph replay used to leave the every-step rule out: it is single-GPU, no
        exchange is attached -- ``capture_train_step`` refuses a world of more than one rank -- so the answer is the same.)"""
        if self._steps % self.STREAMK_CHECK_EVERY == 0 or self._flat_ar is not None:
            self.check_streamk()
        self._steps += 1

    def _adam_state(self):
        """Adam's second moment, allocated (zero) on first use and made known to the context."""
        if self.exp_avg_sq is None:
            self.exp_avg_sq = torch.zeros_like(self.params)
            self._bind_optim_state()
        return self.exp_avg_sq

    def _bind_optim_state(self):
        if self._group_of is None:
            self._group_of = torch.full((self.n_params,), _lib.OPTIM_NO_GRAD, dtype=torch.uint8, device=self.device)
        _lib.check(self.lib.pevit_set_optim_state(self._ctx, _lib.ptr(self.exp_avg_sq), _lib.ptr(self._group_of)), "pevit_set_optim_state")

    def optimizer_step(self, plan: "OptimPlan", grad_scale=1.0, _pipelined=False):
        """``optimizer.step()`` of the optimizer ``plan`` describes (torch.optim.Adam / AdamW, or SGD whose groups differ) as one
        launch of the fused kernel (csrc/optim.hip) over the flat buffer.  ``exp_avg`` lives in ``self.momentum``, ``exp_avg_sq`` in
        ``self.exp_avg_sq``; the Adam step ``t`` is this engine's count of optimizer calls since ``reset_optimizer()`` (there is
        no device-side counter): an update that a raised error word withholds still counts, so after ``clear_streamk_error()``
        the bias corrections are those of the call count, one ahead of the updates applied, per withheld step.  The state belongs to one optimizer kind: a plan of another kind raises until
        ``reset_optimizer()``.  Error words, the periodic check and ``dp_flush()`` behave as in ``sgd_step``."""
        if not _pipelined:
            self.dp_flush()
        prior = self._optim_kind or ("sgd" if self._steps else None)
        if prior is not None and prior != plan.kind:
            raise _lib.PevitError(f"optimizer_step: the optimizer state belongs to {prior!r}, the plan is {plan.kind!r}; call "
                                  f"reset_optimizer() first")
        n = len(plan.groups)
        if not 1 <= n <= _lib.OPTIM_MAX_GROUPS:
            raise _lib.PevitError(f"optimizer_step: {n} parameter groups (1 to {_lib.OPTIM_MAX_GROUPS} are supported)")
        if plan.kind != "sgd":
            self._adam_state()
        host = plan.group_of
        seen = (host, host._version)            # the same tensor, not written since: nothing to compare
        if self._group_of_seen is None or seen[0] is not self._group_of_seen[0] or seen[1] != self._group_of_seen[1]:
            if host.dtype != torch.uint8 or host.numel() != self.n_params:
                raise _lib.PevitError(f"optimizer_step: group_of must hold {self.n_params} uint8 entries")
            if self._group_of_host is None or not torch.equal(host, self._group_of_host):      # membership changed: the one upload
                if self._group_of is None:
                    self._bind_optim_state()
                self._group_of.copy_(host)
                self._group_of_host = host.clone()
            self._group_of_seen = seen
        groups = (_lib.PevitOptimGroup * n)()
        for dst, g in zip(groups, plan.groups):
            dst.lr, dst.weight_decay, dst.momentum = g["lr"], g["weight_decay"], g.get("momentum", 0.0)
            dst.beta1, dst.beta2, dst.eps = g.get("beta1", 0.0), g.get("beta2", 0.0), g.get("eps", 0.0)
            dst.nesterov = int(bool(g.get("nesterov", False)))
        _lib.check(self.lib.pevit_optim_step(self._ctx, _lib.stream_ptr(), _lib.OPTIM_KINDS[plan.kind], groups, n,
                                             self._steps + 1, grad_scale, int(self._steps == 0)), "pevit_optim_step")
        self._optim_kind = plan.kind
        self._after_update()

    def _clip_grad_norm(self, max_norm, grad_scale=1.0, _pipelined=False):
        """(Public as ``engine_optim.clip_grad_norm(engine, ...)``: the class surface of ``HipEngine`` is a recorded one.)
        ``torch.nn.utils.clip_grad_norm_(parameters, max_norm)`` (norm_type 2, f32) on ``self.grads`` as two launches on the
        current stream, no host read (``pevit_clip_grad_norm``): the tensors whose ``.grad`` is None in torch (``grad_mask``) are
        neither counted nor touched.  ``grad_scale``: the update's factor (1 / world where the buffer holds the sum over the
        ranks); it scales the norm only, the buffer is multiplied by the clip coefficient alone.  Returns ``last_grad_norm``: the
        0-dim device view of the norm BEFORE clipping, not synchronised (the next clip overwrites it)."""
        if not _pipelined:
            self.dp_flush()
        _lib.check(self.lib.pevit_clip_grad_norm(self._ctx, _lib.stream_ptr(), float(max_norm), float(grad_scale),
                                                 _lib.ptr(self._clip_scratch)), "pevit_clip_grad_norm")
        return self.last_grad_norm

    def _update(self, optimizer, lr, momentum, weight_decay, grad_scale, nesterov, _pipelined=False):
        """The step's one dispatch point between the plain-SGD kernel and a planned optimizer; with ``self.max_grad_norm`` set the
        gradients are clipped right in front of it, on the stream the update runs on (under data parallelism: behind the exchange,
        on the norm of the averaged gradient).  Every caller -- plain ``train_step`` and the three DP schedules -- comes through here."""
        if self.max_grad_norm is not None:
            self._clip_grad_norm(self.max_grad_norm, grad_scale, _pipelined=_pipelined)
        if optimizer is not None:
            return self.optimizer_step(optimizer, grad_scale, _pipelined=_pipelined)
        self.sgd_step(lr, momentum, weight_decay, grad_scale, nesterov, _pipelined=_pipelined)

    def check_streamk(self):
        """Stream-K GEMMs hand partial tiles between workgroups inside one launch; a consumer that never saw its
        producer gives up after ~1 s and raises an error word instead of hanging.  Fails loudly if that happened, and says how
        many optimizer updates the fused SGD kernel withheld since.  The word is NOT cleared here: every later update is
        withheld and every later check raises again until the caller acknowledges with ``clear_streamk_error()``."""
        word, skipped = C.c_uint(), C.c_uint()
        _lib.check(self.lib.pevit_streamk_status(self._ctx, _lib.stream_ptr(), C.byref(word), C.byref(skipped)), "pevit_streamk_status")
        if self._flat_ar is not None:       # the DP exchange's error word (updates were withheld on device while raised)
            self._flat_ar.check(stream=self._flat_ar_stream)
        if word.value:
            raise _lib.PevitError(f"stream-K GEMM hand-off timed out: the logits / loss returned since are invalid and "
                                  f"{skipped.value} optimizer update(s) were withheld on device (parameters and momentum are those "
                                  f"of the last good step); call clear_streamk_error() to resume")

    def clear_streamk_error(self) -> bool:
        """Acknowledge a stream-K error (clears the device word and the withheld-update counter); True if one was pending."""
        rc = self.lib.pevit_streamk_error(self._ctx, _lib.stream_ptr())
        if rc < 0:
            raise _lib.PevitError("pevit_streamk_error failed")
        return rc > 0

    def reset_optimizer(self):
        self.dp_flush()
        self._steps = 0
        self._optim_kind = None
        self.momentum.zero_()
        if self.exp_avg_sq is not None:
            self.exp_avg_sq.zero_()

    def reset_run(self):
        """State a fresh ``Classifier`` would have, with the frozen backbone left resident (the
        reference rebuilds everything for each of its ~90 sweep runs).  Clears both optimizer moments."""
        self.dp_flush()
        self.reset_optimizer()
        self.params.zero_(); self.grads.zero_()
        self.running_mean.zero_(); self.running_var.fill_(1.0)

    # ---- whole-step HIP graph -----------------------------------------------------
    def capture_train_step(self, images, labels, lr=None, momentum=0.9, weight_decay=0.0, bn_training=True, nesterov=False,
                           optimizer=None):
        """Capture ``forward_backward + sgd_step`` on THESE buffers (pointers, batch, hyper-parameters and BatchNorm mode are baked
        in) into a HIP graph and return a callable that replays it: one hipGraphLaunch instead of ~200 kernel launches from the
        C call.  The step counter, the periodic error-word check and the results (``self._logits``, ``self._loss``) behave as in
        ``train_step``.  At least one eager step must have run (the first SGD step has no momentum buffer to read, and the
        library's one-time attribute calls are not stream operations).  Same kernels, same order: bit-identical to eager
        (tests/test_gpu_mirror.py::test_graph_replay_equals_eager).  Measured: profiles/r05_graph_capture.md.
        Plain SGD only: the Adam step count ``t`` is kept by the host and reaches the kernel by value, so a captured launch would
        replay one fixed ``t``; an ``optimizer`` plan (``optimizer_step``) raises here until a device-side counter exists.
        With ``self.max_grad_norm`` set at capture time the two launches of the clip are captured between the backward and the
        update, the bound baked in like the other hyper-parameters (the clip coefficient lives on the device, so a replay clips by
        the norm of ITS gradients)."""
        if optimizer is not None:
            raise _lib.PevitError("capture_train_step captures the plain-SGD step only: the planned optimizers (Adam, AdamW, "
                                  "per-group SGD) take their step count and hyper-parameters by value on every launch")
        if lr is None:
            raise TypeError("capture_train_step: lr is required")
        if self._steps == 0:
            raise _lib.PevitError("capture_train_step: run one eager train_step first (first-step flag, one-time kernel attributes)")
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise _lib.PevitError("capture_train_step is a single-GPU tool: the captured step has no gradient exchange")
        # leaves the pipelined schedule altogether: a step gate still attached to the context would bake a wait on an event
        # recorded OUTSIDE the capture (and the gated zero_grads path) into the graph
        self.dp_pipeline_off()
        B = images.shape[0]
        if self._needs_resize(images):
            raise _lib.PevitError("capture_train_step: the batch needs the input resize, which is not part of the captured step: "
                                  "capture on resize_u8(images) copied to a buffer of your own")
        fn = self._train_fn(images, self._check_batch(images, labels))
        flags = 2 if nesterov else 0
        logits, loss = self._logits[:B], self._loss
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
                _lib.check(fn(self._ctx, _lib.stream_ptr(), _lib.ptr(images), _lib.ptr(labels), _lib.ptr(self.running_mean),
                              _lib.ptr(self.running_var), int(bn_training), _lib.ptr(logits), _lib.ptr(loss), B),
                           "pevit_train_forward_backward (capture)")
                if self.max_grad_norm is not None:
                    _lib.check(self.lib.pevit_clip_grad_norm(self._ctx, _lib.stream_ptr(), float(self.max_grad_norm), 1.0,
                                                             _lib.ptr(self._clip_scratch)), "pevit_clip_grad_norm (capture)")
                _lib.check(self.lib.pevit_sgd_step(self._ctx, _lib.stream_ptr(), lr, momentum, weight_decay, 1.0, flags),
                           "pevit_sgd_step (capture)")
        torch.cuda.current_stream(self.device).wait_stream(side)
        keep = (images, labels)                     # the graph reads these addresses on every replay

        def replay():
            self._begin_forward((), flush=False)
            graph.replay()
            self._after_update()
            return logits, loss
        replay.graph, replay.buffers = graph, keep
        return replay
