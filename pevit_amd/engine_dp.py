"""The data-parallel schedules of ``HipEngine``: how the flat gradient buffer -- the only thing that crosses xGMI -- is exchanged
between the fused forward/backward call and the update ("single", "staged", "pipelined"), the exchange's timing hooks, and what
keeps replicas equal.  A mixin: its state (``_pipe``, ``_xt``, ``_flat_ar``, ``_flat_ar_stream``, ``_dp_streamk_off``,
``_dfeat_buf``) is declared in ``HipEngine.__init__``."""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import torch

from . import _lib, dp


_DONE = SimpleNamespace(wait=lambda: None)      # what _exchange returns for a collective already on the current stream


class DpMixin:
    #: how the DP step exchanges the gradients: "single" = the fused forward/backward call, then ONE all-reduce of the whole
    #: flat buffer (406 KB for KAdaptation) | "staged" = the backward cut into stages with three overlapped buckets (rounds 2-4) |
    #: "pipelined" (train_step only) = "single" with the exchange + SGD on a second stream under the NEXT step's stem.
    #: Round 5 made "single" the default: the exchange is latency-bound at this size, so what the staged route can hide is the
    #: transfer of two of its three buckets, while the LAST bucket's latency is exposed either way -- and the staging itself (a
    #: second reduce / chain / rule-sum group, three round trips through the collective's stream at ~74 us each, stream-K off)
    #: costs 3.6 % of the step on one rank against 0.2 % for one in-stream exchange behind the fused call
    #: (bench.py --dp-route; profiles/r05_dp_single_exchange.md).
    dp_exchange_mode = "single"

    def _train_step_dp(self, images, labels, lr, momentum, weight_decay, bn_training, process_group, world_size, nesterov,
                       logits_out, loss_out, optimizer):
        """``train_step`` on more than one rank: the schedule ``dp_exchange_mode`` names, 1/world folded into the update."""
        if self.dp_exchange_mode == "pipelined":
            return self._train_step_pipelined(images, labels, lr, momentum, weight_decay, bn_training, process_group, world_size,
                                              nesterov, logits_out, loss_out, optimizer)
        logits, loss = self.forward_backward_dp(images, labels, bn_training, process_group)
        if logits_out is not None:
            logits_out.copy_(logits)
        if loss_out is not None:
            loss_out.copy_(loss)
        self._update(optimizer, lr, momentum, weight_decay, 1.0 / world_size, nesterov)
        return logits, loss

    # ---- DP with the exchange under the next step's stem (round 5) ----------------------------------------------------------------
    def _train_step_pipelined(self, images, labels, lr, momentum, weight_decay, bn_training, process_group, world_size, nesterov,
                              logits_out, loss_out, optimizer=None):
        """``dp_exchange_mode = "pipelined"``: the fused forward/backward call on the current stream; the all-reduce of the flat
        gradient buffer and the fused SGD kernel on a SECOND stream behind it; the next fused call runs its stem (patch gather,
        patch embedding, ln_pre: ~70 us that read no trainable parameter) and only then waits, on the device, for the update
        (``pevit_set_step_gate``).  The exchange's latency and the cross-stream hand-overs around the collective leave the critical
        path.  Same kernels, same order of arithmetic as the other modes: bit-identical results (tests/test_gpu_dp.py).
        The caller's obligations: every step of a run goes through ``train_step`` on ONE stream; ``dp_flush()`` before anything
        else reads parameters / momentum / gradients or launches on them (validation, ``state_dict``, another mode) -- the
        engine's own entry points that do so call it."""
        cur = torch.cuda.current_stream(self.device)
        st = self._pipe
        if st is None:
            st = self._pipe = {"stream": torch.cuda.Stream(self.device), "grads": torch.cuda.Event(), "params": torch.cuda.Event(),
                               "open": False}
            st["params"].record(cur)                       # (creates the event: nothing to wait for before the first step)
            _lib.check(self.lib.pevit_set_step_gate(self._ctx, C.c_void_p(st["params"].cuda_event)), "pevit_set_step_gate")
        st["open"] = True
        logits, loss = self.forward_backward(images, labels, bn_training, logits_out, loss_out)     # waits for st["params"] behind its stem
        st["grads"].record(cur)
        with torch.cuda.stream(st["stream"]):
            st["stream"].wait_event(st["grads"])
            self._exchange_timed(self.grads, process_group)
            self._update(optimizer, lr, momentum, weight_decay, 1.0 / world_size, nesterov, _pipelined=True)
            st["params"].record(st["stream"])
        return logits, loss

    def dp_flush(self):
        """Pipelined DP: make the current stream wait for the last exchange + update (no-op otherwise)."""
        st = self._pipe
        if st is not None and st["open"]:
            torch.cuda.current_stream(self.device).wait_event(st["params"])
            st["open"] = False

    def dp_pipeline_off(self):
        """Leave the pipelined schedule: flush, detach the step gate from the context, drop the second stream."""
        self.dp_flush()
        if self._pipe is not None:
            _lib.check(self.lib.pevit_set_step_gate(self._ctx, None), "pevit_set_step_gate")
            self._pipe = None

    # ---- how long the exchange takes on the device (bench.py N > 1: `exchange_us_per_step`) ---------------------------------------
    def time_exchange(self, on: bool = True):
        """Bracket every gradient exchange of the DP step with a pair of events on the stream it is enqueued on (single / staged:
        the compute stream -- for staged the pair brackets the WAITS at the end of the backward, i.e. the part of the three
        asynchronous all-reduces that the backward did not hide; pipelined: the second stream).  ``exchange_times_us()`` reads
        them back."""
        self._xt = [] if on else None

    def _xt_pair(self):
        if self._xt is None:
            return None
        self._xt.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
        return self._xt[-1]

    def exchange_times_us(self):
        """Microseconds of every bracketed exchange since time_exchange(True) (synchronises the device)."""
        torch.cuda.synchronize(self.device)
        return [a.elapsed_time(b) * 1e3 for a, b in (self._xt or [])]

    def use_flat_allreduce(self, process_group=None):
        """Exchange the gradient buckets with pevit_allreduce_flat (dp.FlatAllReduce: IPC-mapped peer mailboxes, copy-engine
        pushes, deterministic local reduction on a side stream) instead of the process group's all-reduce."""
        self._flat_ar = dp.FlatAllReduce(self.n_params, group=process_group, device=self.device)
        self._flat_ar_stream = torch.cuda.Stream(self.device)
        # a bucket whose exchange gave up (a peer never arrived, sizes disagree) must not reach the parameters: the fused SGD
        # kernel reads the all-reduce's error word next to the stream-K one and withholds the update while either is raised
        _lib.check(self.lib.pevit_set_external_poison(self._ctx, C.c_void_p(self._flat_ar.error_word())), "pevit_set_external_poison")
        return self._flat_ar

    def _exchange(self, view, process_group, in_stream=False):
        """Start the sum all-reduce of one gradient bucket; returns something with .wait().
        in_stream: nothing is to run beside the exchange (the single-exchange schedule): the SYNCHRONOUS form of the collective,
        which this torch enqueues on the CURRENT stream.  Measured on a 1-rank RCCL group (scripts/r5_dp_hosttime.py): a round trip
        through a second stream -- what ``async_op=True`` + ``wait()`` is, with or without a collective on it -- costs 74 us of
        device time per step on this platform, the synchronous call 7 us."""
        import torch.distributed as dist
        ar = self._flat_ar
        if ar is None and in_stream:
            dist.all_reduce(view, op=dist.ReduceOp.SUM, group=process_group)
            return _DONE
        if ar is None:
            return dist.all_reduce(view, op=dist.ReduceOp.SUM, group=process_group, async_op=True)
        if in_stream:
            ar.all_reduce(view, stream=torch.cuda.current_stream(self.device))
            return _DONE
        cur, side = torch.cuda.current_stream(self.device), self._flat_ar_stream
        ready = torch.cuda.Event(); ready.record(cur)
        side.wait_event(ready)                          # the bucket's gradients are final
        ar.all_reduce(view, stream=side)
        done = torch.cuda.Event(); done.record(side)
        return SimpleNamespace(wait=lambda: torch.cuda.current_stream(self.device).wait_event(done))

    def _exchange_timed(self, view, process_group):
        """The in-stream exchange of the single and pipelined schedules between its pair of timing events, if any, all on the
        current stream (pipelined: the second one)."""
        xt = self._xt_pair()
        if xt: xt[0].record()
        self._exchange(view, process_group, in_stream=True).wait()
        if xt: xt[1].record()

    def forward_backward_dp(self, images, labels, bn_training=True, process_group=None, mode=None):
        """forward_backward() followed by the gradient exchange; leaves the SUM over ranks in ``self.grads``.
        mode "single" (default, ``dp_exchange_mode``): the fused call, then one all-reduce of the flat gradient buffer.
        mode "staged": the call cut into stages so that the exchange overlaps the backward -- three buckets of the flat buffer, each
        all-reduced asynchronously as soon as its gradients are final:  head (after the head backward) | blocks L/2..L-1 (after
        the upper half of the tower backward) | shared rules + blocks 0..L/2-1 (at the end).  Same kernels in the same order as
        the fused call either way, so a single rank reproduces forward_backward() bit for bit."""
        mode = mode or self.dp_exchange_mode
        self.dp_flush()
        if mode == "pipelined":
            raise ValueError("forward_backward_dp: the pipelined schedule spans the optimizer step -- use train_step")
        if mode == "single":
            if self._dp_streamk_off:        # (a staged step before this one switched it off)
                self.tune("gemm_streamk", 1); self._dp_streamk_off = False
            logits, loss = self.forward_backward(images, labels, bn_training)
            self._exchange_timed(self.grads, process_group)
            return logits, loss
        if mode != "staged":
            raise ValueError(f"forward_backward_dp: unknown mode {mode!r}")
        B = images.shape[0]
        images = self._input(images)
        self._check_batch(images, labels)
        if not self._dp_streamk_off:
            # the RCCL kernels of the overlapped all-reduce share the CUs with the second half of the backward: stream-K's
            # hand-off assumes all its workgroups are co-resident, so under DP the plain tilings are used instead
            self.tune("gemm_streamk", 0)
            self._dp_streamk_off = True
        self.zero_grad()
        feat = self.visual_forward(images, save=True)
        logits, loss, dfeat = self.head_forward_backward(feat, labels, bn_training, out=(self._logits[:B], self._loss, self._dfeat(B)))
        L, mid = self.arch.layers, self.arch.layers // 2
        cut = self.lib.pevit_param_layer_offset(self._ctx, mid)
        work = [self._exchange(self.grads[self.n_tower:], process_group)]
        if self.n_tower == 0:                                  # frozen tower (linear probe): nothing below the head trains
            work[0].wait()
            return logits, loss
        if mid > 0:
            _lib.check(self.lib.pevit_visual_backward_part(self._ctx, _lib.stream_ptr(), _lib.ptr(dfeat), B, L, mid),
                       "pevit_visual_backward_part")
            work.append(self._exchange(self.grads[cut:self.n_tower], process_group))
            _lib.check(self.lib.pevit_visual_backward_part(self._ctx, _lib.stream_ptr(), None, B, mid, 0),
                       "pevit_visual_backward_part")
            work.append(self._exchange(self.grads[:cut], process_group))
        else:
            self.visual_backward(dfeat)
            work.append(self._exchange(self.grads[:self.n_tower], process_group))
        xt = self._xt_pair()
        if xt: xt[0].record()
        for w in work:
            w.wait()
        if xt: xt[1].record()
        return logits, loss

    def _dfeat(self, B):
        if self._dfeat_buf is None or self._dfeat_buf.shape[0] < B:
            self._dfeat_buf = torch.empty((max(B, self.max_batch), self.arch.embed_dim), dtype=torch.float32, device=self.device)
        return self._dfeat_buf[:B]

    def sync_replicas(self, process_group=None, src: int = 0):
        """Make every rank's trainable state identical to rank ``src``'s (parameters, momentum / exp_avg, exp_avg_sq, BatchNorm
        running statistics, step counter semantics): call once after the engines have been loaded and before the first DP step.
        ``exp_avg_sq`` travels only where it exists, that is after the first Adam / AdamW step, which every rank takes together;
        before it the buffer is unallocated on all of them and starts from zero, so a plain-SGD run allocates and sends nothing more
        than it did."""
        self.dp_flush()
        import torch.distributed as dist
        state = [self.params, self.momentum, self.running_mean, self.running_var]
        if self.exp_avg_sq is not None:
            state.append(self.exp_avg_sq)
        for t in state:
            dist.broadcast(t, src=src, group=process_group)

    def average_bn_buffers(self, process_group=None):
        """BatchNorm running statistics follow the LOCAL shards; average them across ranks before validation or a
        checkpoint (dp.average_bn_buffers)."""
        self.dp_flush()
        dp.average_bn_buffers(self.running_mean, self.running_var, process_group)
