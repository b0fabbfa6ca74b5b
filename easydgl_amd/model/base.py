"""Mirror of src/model/Base.py:Sequential — the model base class (flags, output bias, loss/eval scaffold)
re-hosted on torch.nn.Module with a flat parameter arena for the fused optimizer."""
from __future__ import annotations

from typing import Dict, List, Optional

import torch
from torch import nn

from .. import ops
from ..module.coding import glorot_uniform_


NEG_SAMPLERS = ("uniform", "popularity", "log_uniform")     # FLAGS.neg_sampler


class _Dense(nn.Module):
    """tf.layers.dense parameters: kernel [in,out] glorot_uniform, bias zeros."""

    def __init__(self, n_in, n_out, gen):
        super().__init__()
        self.kernel = nn.Parameter(glorot_uniform_(torch.empty(n_in, n_out), gen))
        self.bias = nn.Parameter(torch.zeros(n_out))


class _LayerNorm(nn.Module):
    """Base.layernorm parameters (Base.py:36-49): beta zeros, gamma ones over the last axis."""

    def __init__(self, n):
        super().__init__()
        self.beta = nn.Parameter(torch.zeros(n))
        self.gamma = nn.Parameter(torch.ones(n))


class _FeedForward(nn.Module):
    """Base.FeedForward([C, C]) (Base.py:70-87): Conv1D(k=1, relu) -> dropout -> Conv1D(k=1) -> dropout -> + input."""

    def __init__(self, C_, gen):
        super().__init__()
        self.inner = _Dense(C_, C_, gen)      # dense/Inner
        self.readout = _Dense(C_, C_, gen)    # dense/Readout


class Sequential(nn.Module):
    """Base.py:90-207.  Reads the same FLAGS fields as the reference (Base.py:92-104)."""

    tf_numpy = True     # tf_values() / tf_gradients() hand float32 numpy arrays out (EasyDGL: tensors on the parameters' device)
    lazy_adam_ok = False     # FLAGS.lazy_adam: only a model whose item backward ADDS into d_item (EasyDGL)
    adam_hparams = (0.9, 0.999, 1e-8)     # (beta1, beta2, epsilon) of tf.train.AdamOptimizer (Base.py:142-144); S2PNM overrides
    static_engine_ok = True  # engine.TrainEngine refuses a model that sets this to False (SASRec, S2PNM: DESIGN 4.17)
    clip_norm = None         # clip_by_global_norm over the whole gradient arena in front of the update (S2PNM.py:87); None: off

    def __init__(self, num_items, FLAGS):
        super().__init__()
        self.num_items = num_items
        self.num_units = FLAGS.num_units
        self.num_heads = FLAGS.num_heads
        self.hidden_dropout_rate = float(getattr(FLAGS, "hidden_dropout_rate", 0.0) or 0.0)
        self.attention_probs_dropout_rate = float(getattr(FLAGS, "attention_probs_dropout_rate", 0.0) or 0.0)
        self.seqslen = FLAGS.seqslen
        self.learning_rate = FLAGS.learning_rate
        self.l2_reg = float(getattr(FLAGS, "l2_reg", 0.0) or 0.0)
        self.num_train_steps = getattr(FLAGS, "num_train_steps", None)
        self.num_warmup_steps = getattr(FLAGS, "num_warmup_steps", None)
        cd = getattr(FLAGS, "compute_dtype", "bf16")
        self.act_dtype = {"bf16": torch.bfloat16, "f32": torch.float32, "fp32": torch.float32}[cd]
        # bitwise reproducible training: every scatter / bin sum of the model's ops runs in its ordered form
        self.deterministic = bool(getattr(FLAGS, "deterministic", False))
        # sampled-softmax training: N > 0 negatives per scored row instead of the softmax over the catalogue
        self.train_negatives = int(getattr(FLAGS, "train_negatives", 0) or 0)
        self.train_neg_seed = int(getattr(FLAGS, "train_neg_seed", 0) or 0)
        self.neg_step = 0       # sampled training steps taken (host side; the `step` key of the lists; travels in checkpoints)
        if self.train_negatives < 0:
            raise ValueError(f"train_negatives={self.train_negatives}: the number of sampled negatives per row (0: full softmax)")
        # one negative list per step, shared by every row: S > 0 ids drawn once per step; a different estimator
        self.shared_negatives = int(getattr(FLAGS, "shared_negatives", 0) or 0)
        if self.shared_negatives < 0 or self.shared_negatives > ops.MAX_SHARED:
            raise ValueError(f"shared_negatives={self.shared_negatives}: the length of the step's shared negative list "
                             f"(0: off, at most {ops.MAX_SHARED})")
        if self.shared_negatives > 0 and self.train_negatives > 0:
            raise ValueError("shared_negatives and train_negatives are both set: one estimator per run (per-row lists, DESIGN "
                             "4.13, or one shared list, DESIGN 4.15)")
        # weighted negatives with the log-Q correction: which distribution the sampled modes draw from
        self.neg_sampler = str(getattr(FLAGS, "neg_sampler", None) or "uniform")
        alpha = getattr(FLAGS, "neg_alpha", None)
        self.neg_alpha = 0.75 if alpha is None else float(alpha)
        if self.neg_sampler not in NEG_SAMPLERS:
            raise ValueError(f"neg_sampler={self.neg_sampler!r}: one of {', '.join(NEG_SAMPLERS)}")
        if self.neg_sampler != "uniform" and self.train_negatives <= 0 and self.shared_negatives <= 0:
            raise ValueError(f"neg_sampler={self.neg_sampler!r} needs train_negatives > 0 or shared_negatives > 0: the full softmax "
                             "draws no negatives")
        # the objective over the sampled slots: softmax, or bce / bpr over the same lists and values
        self.sampled_loss = str(getattr(FLAGS, "sampled_loss", None) or "softmax")
        if self.sampled_loss not in ops.LOSS_FORMS:
            raise ValueError(f"sampled_loss={self.sampled_loss!r}: one of {', '.join(ops.LOSS_FORMS)}")
        if self.sampled_loss != "softmax" and self.train_negatives <= 0 and self.shared_negatives <= 0:
            raise ValueError(f"sampled_loss={self.sampled_loss!r} needs train_negatives > 0 or shared_negatives > 0: the objective is "
                             "defined over sampled negatives, the full softmax draws none")
        self._neg_dist = None   # ops.NegDist over [1, _negatives_hi()): set_negative_weights (log_uniform: built at the first draw)
        # lazy row-wise Adam for the item table: the table's gradient lands in place in the gradient arena and the
        # optimizer walks only the rows the step used
        self.lazy_adam = bool(getattr(FLAGS, "lazy_adam", False))
        if self.lazy_adam and self.train_negatives <= 0 and self.shared_negatives <= 0:
            raise ValueError("lazy_adam needs train_negatives > 0 or shared_negatives > 0: the full softmax has a dense table gradient (every row of the "
                             "catalogue is scored), there are no untouched rows to skip")
        if self.lazy_adam and not self.lazy_adam_ok:
            raise ValueError(f"lazy_adam: {type(self).__name__} is not supported — its item backward (edgl_embed_pos_bwd_*) "
                             "overwrites d_item instead of adding into it; only EasyDGL runs the mode")
        self._lazy_pending: list = []     # (seqs_i, labels, candidates) of the train_loss calls since the last optimizer step
        self._arena: Optional[torch.Tensor] = None
        self.pad = (0, 0)       # (dh_pad, dh_true) of a channel-padded model (a head dim the kernels do not tile)
        self._metrics = None
        # hand-over state between this model and the static engines that train it (engine.TrainEngine)
        self._state_ahead = False        # the step counters already hold the NEXT step's values (settle_state undoes it)
        self._state_pinned = False       # a captured graph keeps the counters' addresses: no engine swaps the buffers any more
        self._table_grad_zero = None     # id of the engine whose optimizer launch left the tied table's / output bias's gradient at zero
        self._l2_parts_owner = None      # id of the engine whose optimizer launch left the sums of squares of the current weights

    # ---- flat parameter arena -------------------------------------------------------------------------
    def finalize(self, device) -> "Sequential":
        """Move to `device` and re-home every parameter as a view of ONE flat f32 arena (plus a flat
        gradient arena, Adam moments and — in bf16 mode — a bf16 shadow refreshed by the optimizer kernel).
        Embedding tables come first so that the l2 segments (coding.py:48-55) are contiguous ranges."""
        self.to(device)
        names = [n for n, _ in self.named_parameters()]
        order = sorted(names, key=lambda n: (0 if n in self.l2_param_names() else 1, names.index(n)))
        params = dict(self.named_parameters())
        total = sum(params[n].numel() for n in order)
        # keep every view 16-byte aligned for the vector loads of the kernels
        offs, o = {}, 0
        for n in order:
            offs[n] = o
            o += (params[n].numel() + 7) // 8 * 8
        total = o
        arena = torch.zeros(total, device=device, dtype=torch.float32)
        # the gradient arena carries 8 trailing floats that are no parameter's gradient: scalars that must travel with the ONE
        # data-parallel all-reduce of a step (TrainEngine: this rank's share of the cross-entropy + TPP loss)
        self._grad_comm = torch.zeros(total + 8, device=device, dtype=torch.float32)
        grad = self._grad_comm[:total]
        for n in order:
            p = params[n]
            view = arena[offs[n]:offs[n] + p.numel()].view(p.shape)
            view.copy_(p.data)
            p.data = view
            p.grad = grad[offs[n]:offs[n] + p.numel()].view(p.shape)
        self._arena, self._grad_arena, self._offsets, self._order = arena, grad, offs, order
        self._plist = [(params[n], params[n].grad) for n in order]   # (parameter, its view of the gradient arena)
        self._adam_m = torch.zeros_like(arena)
        self._adam_v = torch.zeros_like(arena)
        self._adam_state = torch.zeros(2, device=device, dtype=torch.int64)
        self._rng_state = torch.tensor([getattr(self, "seed", 9876), 0], device=device, dtype=torch.int64)
        segs: List[int] = []
        for n in self.l2_param_names():
            segs += [offs[n], offs[n] + params[n].numel()]
        self._l2_seg = torch.tensor(segs, device=device, dtype=torch.int64) if segs else None
        self._shadow = None
        if self.act_dtype != torch.float32:
            self._shadow = torch.empty(total, device=device, dtype=self.act_dtype)
            self.sync_shadow()
        if self.lazy_adam:
            # the item table's range of the arena and the claim words of edgl_adam_rows (one per table row; not saved in
            # checkpoints: a zeroed stamp is right after a restore)
            tab = self.item_embs.lookup_table
            lo = (tab.data_ptr() - arena.data_ptr()) // 4
            self._lazy_range = (lo, lo + (tab.numel() + 7) // 8 * 8)
            self._lazy_grad = tab.grad      # (the table's view of the gradient arena, the object _plist holds)
            self._stamp = torch.zeros(tab.shape[0], device=device, dtype=torch.int32)
            self._lazy_pending = []
        # operator modules (module/coding.py, module/temporal.py) read parameters through the owning model's compute copy
        for mod in self.modules():
            if mod is self:
                continue
            if "compute" in mod.__dict__:
                mod.compute = self.compute
            if "act_dtype" in mod.__dict__:
                mod.act_dtype = self.act_dtype
        return self

    def l2_param_names(self) -> List[str]:
        return []

    def sync_shadow(self) -> None:
        """Refresh the low-precision compute copies after the f32 masters were changed outside adam_step."""
        self._l2_parts_owner = None      # (the weights were rewritten: no engine's sums of squares describe them any more)
        if self._shadow is not None:
            ops.cast_to(self._arena, self.act_dtype, out=self._shadow)

    def compute(self, p: torch.Tensor) -> torch.Tensor:
        """Tensor the kernels read for parameter `p`: the master (f32 mode) or its bf16 shadow view."""
        if self._arena is None:
            raise RuntimeError("call model.finalize(device) before running the model")
        if self._shadow is None:
            return p
        off = (p.data_ptr() - self._arena.data_ptr()) // 4
        return self._shadow[off:off + p.numel()].view(p.shape)

    def zero_grad_arena(self) -> None:
        """Zero the whole gradient arena.  With lazy_adam this also restores the mode's invariant after an
        interrupted step — the item table's view is all zeros between steps — and forgets the lists of that step."""
        self._table_grad_zero = None
        self._lazy_pending = []
        self._grad_arena.zero_()

    def detach_grads(self) -> None:
        """Before an autograd backward of a training step: with `.grad` unset autograd hands every parameter the gradient tensor
        an op produced instead of launching one `+=` kernel per parameter into the arena views."""
        for p, _ in self._plist:
            p.grad = None

    def collect_grads(self) -> None:
        """After that backward: copy the gradients into the flat arena with ONE multi-tensor launch and restore the views.  With
        lazy_adam the item table's range is neither zero-filled nor copied: its gradient was added in place."""
        src, dst = [], []
        lazy_view = self._lazy_grad if self.lazy_adam else None
        for p, view in self._plist:
            g = p.grad
            if view is lazy_view:
                if g is not None:
                    raise RuntimeError("lazy_adam: an op returned a dense gradient for the item table (its gradient is added in "
                                       "place into the gradient arena: pass d_table_out)")
            elif g is None:
                view.zero_()
            else:
                src.append(g)
                dst.append(view)
            p.grad = view
        if dst:
            torch._foreach_copy_(dst, src)

    def graphed_train_step(self, features: Dict[str, torch.Tensor], labels: torch.Tensor, warmup: int = 2):
        """One `train_step` captured into a HIP graph on static copies of the batch: returns step(features, labels) -> loss
        (device scalar) that copies the new batch in and replays ~170 kernel launches as one submission.  Everything a step
        needs lives on the device (dropout step counter, Adam step count), so replays advance like eager steps.  The `warmup`
        eager steps that precede the capture are real optimizer steps."""
        if self.train_negatives > 0:      # (the lists are keyed by a host-side step count: a replay would draw one list for ever)
            raise ValueError("graphed_train_step: a model with train_negatives > 0 (sampled-softmax training, DESIGN 4.13) trains "
                             "through train_step; its step is not captured into a graph")
        if self.shared_negatives > 0:
            raise ValueError("graphed_train_step: a model with shared_negatives > 0 (sampled-softmax training, DESIGN 4.15) trains "
                             "through train_step; its step is not captured into a graph")
        static_f = {k: v.clone() for k, v in features.items()}
        static_l = labels.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        warm_loss = None
        with torch.cuda.stream(side):
            for _ in range(warmup):
                warm_loss = self.train_step(static_f, static_l).clone()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self._state_pinned = True      # (the captured launches keep the step counters' addresses: engine.TrainEngine does not swap them)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            loss = self.train_step(static_f, static_l)

        def step(f, l):
            for k, buf in static_f.items():
                buf.copy_(f[k])
            static_l.copy_(l)
            graph.replay()
            return loss
        step.graph = graph
        step.warmup_loss = warm_loss   # loss of the last eager warm-up step (a real optimizer step on the capture batch)
        return step

    # ---- the variable table and channel padding --------------------------------------------------------------------------------
    # A model lists its variables ONCE, in _pad_specs(): (TF name, parameter, per-axis index map reference -> stored or None for an
    # axis kept whole, initialiser of the reference-shaped variable).  tf_values() / tf_gradients() / load_tf_variables() /
    # padded_leak() / _init_padded() / mask_padded_grads() below are derived from that list and speak the reference's shapes.
    # A head dim the attention kernels do not tile (they take 16 / 32 / 64 / 128; the reference's own default is --num_units 50
    # --num_heads 1, main.py:35-37) runs at the next supported head dim with ZERO-PADDED channels: every parameter is stored at the
    # padded width, head h's true channels sit at [h * dh_pad, h * dh_pad + dh_true), the padded rows / columns are zero and stay
    # zero (the projections' padded columns, the dense layers' padded rows and columns and the tables' padded columns are 0, the
    # LayerNorms take their moments over the real channels and return nothing into the padded ones); the score scale 1 / sqrt(dh)
    # and coding.py's sqrt(num_units) are those of the TRUE width.  What is not zero on a padded entry by itself (rounding residue
    # of a softmax backward's row sums against TGAT's constant time code, the intensity MLP's padded hidden units) is zeroed by
    # mask_padded_grads in front of every optimizer launch.  The index maps come from _cmap() / _mlp_maps(); without padding they
    # are the identity (plus the offset of a column block), so an unpadded model is the trivial case of the same code.
    def _setup_channel_pad(self, who: str, max_pad_dim: int = 128) -> None:
        from ..module import temporal as T
        self.width_true = self.num_units
        self.pad, self.qk_scale = (0, 0), 0.0
        H = self.num_heads
        if H <= 0 or self.num_units % H:
            raise ValueError(f"{who}: num_units={self.num_units} must be a multiple of num_heads={H}")
        dht = self.num_units // H
        if dht in T.SUPPORTED_HEAD_DIMS or dht > max_pad_dim:
            return
        dhp = next(d for d in T.SUPPORTED_HEAD_DIMS if d >= dht)
        if self.lazy_adam:
            raise ValueError(f"lazy_adam: {who} with head dim {dht} runs channel-padded at {dhp}; mask_padded_grads would need its "
                             "flat index over the item table, which the lazy mode never walks — choose a head dim of "
                             f"{T.SUPPORTED_HEAD_DIMS}")
        self.pad = (dhp, dht)
        self.num_units = H * dhp
        self.qk_scale = float(dht) ** -0.5

    def _finish_pad(self, gen) -> None:
        """End of a constructor: a padded model hands its attention units the true score scale and redraws its variables."""
        if self.pad[0]:
            for blk in self.layers:
                blk.attention.qk_scale = self.qk_scale
            self._init_padded(gen)

    def _head_dims(self):
        """(stored, reference) head dim."""
        return self.pad if self.pad[0] else (self.num_units // self.num_heads,) * 2

    def _cmap(self, blocks: int = 1) -> torch.Tensor:
        """True channel -> stored channel, for `blocks` concatenated [C]-wide column blocks (K | V, item | position ...)."""
        dhp, dht = self._head_dims()
        c = torch.arange(self.width_true)
        one = (c // dht) * dhp + (c % dht)
        return torch.cat([one + k * self.num_units for k in range(blocks)])

    def _mlp_maps(self):
        """Maps of the intensity MLP (temporal.BiMAU / MAU): its input rows (dh channels + the span), its hidden units (e, u) and
        the u axis of its output weights."""
        dhp, dht = self._head_dims()
        j = torch.arange(dht * self.num_events)
        return torch.cat([torch.arange(dht), torch.tensor([dhp])]), (j // dht) * dhp + (j % dht), torch.arange(dht)

    def _pad_specs(self):
        raise NotImplementedError

    @staticmethod
    def _spec_index(t, maps):
        """Index of the reference-shaped variable inside the stored tensor `t`: the outer product of the mapped axes, an axis kept
        whole as a slice (a million-row table is not indexed element by element)."""
        mapped = [m.to(t.device) for m in maps if m is not None]
        grid = iter(torch.meshgrid(*mapped, indexing="ij") if mapped else ())
        return tuple(slice(None) if m is None else next(grid) for m in maps)

    @staticmethod
    def _spec_shape(p, maps):
        return tuple(p.shape[a] if m is None else len(m) for a, m in enumerate(maps))

    @torch.no_grad()
    def _init_padded(self, gen) -> None:
        """The reference's initialisers on the TRUE shapes (glorot limits of the true fans), scattered into zeroed padded storage.
        Draws from `gen` in the order of the table."""
        import numpy as np
        specs = self._pad_specs()
        for _, p, _, _ in specs:
            p.data.zero_()
        for _, p, maps, kind in specs:
            shp = self._spec_shape(p, maps)
            if kind == "glorot":
                v = glorot_uniform_(torch.empty(shp), gen)
            elif kind == "normal":         # temporal.py:393 N(0, 0.02): BiMAU's QKVT kernel
                v = torch.randn(shp, generator=gen) * 0.02
            elif kind == "ones":
                v = torch.ones(shp)
            elif kind == "linspace9":      # coding.py:104-108 TimeFunctionCoding.basis_freq
                v = torch.from_numpy(np.linspace(0, 9, shp[0]).astype(np.float32))
            else:
                v = torch.zeros(shp)
            p.data[self._spec_index(p.data, maps)] = v.to(p.device, p.dtype)

    def mask_padded_grads(self) -> None:
        """Zero every gradient entry of a padded row / column (see above); a model without padding: nothing.  ONE index_fill_ on
        the flat gradient arena (the padded entries of every parameter as one int64 index, built once) — a launch per (parameter,
        axis) was dozens of tiny kernels in front of every optimizer step of a 3-block model, captured into the graph step too."""
        if not self.pad[0]:
            return
        plan = getattr(self, "_pad_mask_plan", None)
        if plan is None:
            real = {}      # parameter -> per axis: set of real indices (None: all)
            for _, p, maps, _ in self._pad_specs():
                cur = real.setdefault(id(p), [p] + [set() if m is not None else None for m in maps])
                for a, m in enumerate(maps):
                    if m is not None:
                        cur[1 + a].update(m.tolist())
            per_param, flat = [], []
            base = self._arena.data_ptr()
            for p, *axes in real.values():
                mask = torch.zeros(p.shape, dtype=torch.bool)
                for a, idxs in enumerate(axes):
                    if idxs is not None:
                        padded = sorted(set(range(p.shape[a])) - idxs)
                        if padded:
                            idx = torch.tensor(padded, dtype=torch.int64)
                            mask.index_fill_(a, idx, True)
                            per_param.append((p, a, idx.to(p.device)))
                pos = torch.nonzero(mask.reshape(-1)).reshape(-1)
                if pos.numel():
                    flat.append(pos + (p.data_ptr() - base) // 4)
            flat_idx = torch.cat(flat).to(self._arena.device) if flat else None
            plan = (flat_idx, per_param)
            self._pad_mask_plan = plan
        flat_idx, per_param = plan
        if flat_idx is None:
            return
        g0, n = self._grad_arena.data_ptr(), self._grad_arena.numel()
        if all(p.grad is not None and g0 <= p.grad.data_ptr() < g0 + 4 * n for p, _, _ in per_param):
            self._grad_arena.index_fill_(0, flat_idx, 0.0)      # (every gradient is its view of the arena: the engine and collect_grads)
            return
        for p, a, idx in per_param:
            if p.grad is not None:
                p.grad.index_fill_(a, idx, 0.0)

    @torch.no_grad()
    def padded_leak(self) -> float:
        """Largest |value| on a padded entry of any parameter (0.0 for a healthy model; tests)."""
        worst = 0.0
        clones = {}
        for _, p, maps, _ in self._pad_specs():
            q = clones.setdefault(id(p), p.detach().clone())
            q[self._spec_index(q, maps)] = 0
        for q in clones.values():
            worst = max(worst, float(q.abs().max()))
        return worst

    @torch.no_grad()
    def _padded_values(self, grad: bool):
        out = {}
        for name, p, maps, _ in self._pad_specs():
            t = p.grad if grad else p
            out[name] = t.detach()[self._spec_index(t, maps)].clone()
        return out

    def _tf_out(self, vals):
        return {k: v.float().cpu().numpy() for k, v in vals.items()} if self.tf_numpy else vals

    def tf_values(self):
        """Reference variable name -> value in the REFERENCE's shape (a copy; channel-padded models strip the padding)."""
        return self._tf_out(self._padded_values(False))

    def tf_gradients(self):
        """Reference variable name -> gradient of the last backward in the reference's shape (a copy; K | V (| T_) kernels that are
        stored as one matrix come back as the reference's dense_1 .. dense_3)."""
        return self._tf_out(self._padded_values(True))

    @torch.no_grad()
    def load_tf_variables(self, values) -> None:
        """`values`: TF variable name (scope `main/` stripped) -> array in the reference's shape, as the oracles' init_params list
        them; any other shape is refused."""
        import numpy as np
        specs = self._pad_specs()
        for _, p, _, _ in specs:
            p.data.zero_()
        for name, p, maps, _ in specs:
            v = torch.as_tensor(np.asarray(values[name]), dtype=torch.float32)
            if tuple(v.shape) != self._spec_shape(p, maps):
                raise ValueError(f"{name}: expected shape {self._spec_shape(p, maps)}, got {tuple(v.shape)}")
            p.data[self._spec_index(p.data, maps)] = v.to(p.device, p.dtype)
        self.sync_shadow()

    def settle_state(self) -> None:
        """The static engine leaves the step counters (dropout step, Adam step / learning rate) of the NEXT step in place behind
        its optimizer kernel — the single-thread update then costs nothing in front of the next step's first kernels
        (engine.TrainEngine._advance_state).  Anything else that reads or advances them (the autograd path's steps, a checkpoint)
        calls this first: the counters go back to "steps taken so far"."""
        self._l2_parts_owner = None      # (whoever settles the counters is about to read or rewrite the state itself)
        self._table_grad_zero = None     # (... or the gradient arena: engine.TrainEngine zero-fills the tied table's gradient again)
        if self._state_ahead:
            self._rng_state[1] -= 1
            self._adam_state[0] -= 1
            self._state_ahead = False

    def optimizer_step(self) -> None:
        """tf.train.AdamOptimizer(lr).minimize (Base.py:142-144) fused over the arena.  The l2 gradient is
        produced by autograd (ops.L2Fn), so no l2 is folded in here."""
        self.settle_state()
        self.mask_padded_grads()     # (channel-padded models; idempotent: every optimizer entry point keeps the padded entries at zero)
        if self.clip_norm is not None:      # (a device scalar: no host synchronisation, graphed_train_step captures it)
            ops.clip_by_global_norm(self._grad_arena, self.clip_norm)
        if self.lazy_adam:
            return self._lazy_optimizer_step()
        ops.adam_step(self._arena, self._grad_arena, self._adam_m, self._adam_v, self.learning_rate, self._adam_state,
                      0.0, None, self._shadow, *self.adam_hparams)

    def _lazy_optimizer_step(self) -> None:
        """FLAGS.lazy_adam: the dense TF-form Adam on the arena ranges in front of and behind the item table — the
        first of them advances the step and leaves its learning rate (edgl_adam_step), the other reads it (edgl_adam_apply) —
        and edgl_adam_rows on the table: the rows named by the (seqs_i, labels, candidates) of the train_loss calls since the last
        step are updated once each and their gradient rows go back to zero; every other row keeps w, m and v bit for bit.
        The l2 gradient of the item table, l2_reg * w, is folded in there (the `l2` argument): only touched rows decay, where
        the dense mode decays every row in every step.  The other l2 tables and the output bias keep the dense update."""
        lo, hi = self._lazy_range
        first = True
        for a, b in ((0, lo), (hi, self._arena.numel())):
            if b <= a:
                continue
            sh = None if self._shadow is None else self._shadow[a:b]
            if first:
                ops.adam_step(self._arena[a:b], self._grad_arena[a:b], self._adam_m[a:b], self._adam_v[a:b], self.learning_rate,
                              self._adam_state, 0.0, None, sh, *self.adam_hparams)
            else:
                ops.adam_apply(self._arena[a:b], self._grad_arena[a:b], self._adam_m[a:b], self._adam_v[a:b], self._adam_state,
                               0.0, None, sh, *self.adam_hparams)
            first = False
        if first:
            raise RuntimeError("lazy_adam: the arena holds nothing but the item table (no range advances the Adam step)")
        tab = self.item_embs.lookup_table
        n = tab.numel()
        shadow = None if self._shadow is None else self._shadow[lo:lo + n].view(tab.shape)
        pending, self._lazy_pending = self._lazy_pending, []
        for ids, labels, cand in pending:      # (one launch per train_loss call; a row named by several is claimed once per step)
            ops.adam_rows(tab.data, self._lazy_grad, self._adam_m[lo:lo + n].view(tab.shape), self._adam_v[lo:lo + n].view(tab.shape),
                          shadow, ids, labels, cand, self._stamp, self._adam_state, self.l2_reg, *self.adam_hparams)

    # ---- Base.py:106-113 ---------------------------------------------------------------------------------
    def make_output_bias(self) -> nn.Parameter:
        """output_bias(inf_pad=True): variable [num_items-1] zeros; the used bias is concat([-1000], var)."""
        return nn.Parameter(torch.zeros(self.num_items - 1))

    # ---- helpers of the models' forward passes ---------------------------------------------------------------
    def _drop(self, rate, stream_id, is_training) -> ops.Drop:
        if not is_training or rate <= 0.0:
            return ops.NO_DROP
        return ops.Drop(rate, self._rng_state, stream_id)

    def _linear(self, x, d: _Dense, act=False):
        return ops.LinearFn.apply(x, d.kernel, d.bias, self.compute(d.kernel), act)

    def _feed_forward(self, y, ff: _FeedForward, i, ids, is_training):
        """Base.FeedForward of block `i` behind its LayerNorm `y` (Base.py:79-86); `ids`: ff_tail's key ids (TGAT.py:70) or None."""
        hd = self.hidden_dropout_rate
        inner = self._linear(y, ff.inner, "relu")                                                            # Base.py:79
        if is_training and hd > 0.0:   # Base.py:80: dropout(inner) — an identity LayerNorm-free path: a scaled copy
            inner = ops.dropout(inner, self._drop(hd, 11 + 4 * i, True))
        out = self._linear(inner, ff.readout)                                                                # Base.py:82
        return ops.ff_tail(out, y, ids, self._drop(hd, 12 + 4 * i, is_training))                             # Base.py:83-86

    @staticmethod
    def _last_pos(ids):
        """Gather index [B, 1] of the last position: the row an evaluation scores."""
        return torch.full((ids.shape[0], 1), ids.shape[1] - 1, device=ids.device, dtype=torch.int64)

    @staticmethod
    def _last_labels(labels):
        return (labels[:, -1] if labels.dim() == 2 else labels).contiguous()

    # ---- Sequential.train (Base.py:119-144) ------------------------------------------------------------------
    def _score_ce(self, rows, labels, candidates=None, shared=None):
        """The cross-entropy of a training step over `rows` [R, C] / `labels` int64 [R]: the softmax over the catalogue
        (ops.ScoreCEFn), or — with `candidates` (int32 [R, N], one list per scored row) or FLAGS.train_negatives = N > 0 — over each
        row's label and its own list (ops.SampledCEFn).  Sampled lists are keyed by (train_neg_seed, neg_step, row);
        train_step advances neg_step, so a resumed run draws the lists the uninterrupted run would have drawn, and calling
        train_loss twice in between scores the same lists.  A range [1, hi) too small for the sampler is refused by the sampler.
        `shared` (int32 [S], one list for every row) or FLAGS.shared_negatives = S > 0: each row's label and the step's ONE list
        (ops.SharedCEFn), drawn once through the same sampler, keyed by (train_neg_seed, neg_step).
        FLAGS.neg_sampler other than "uniform" (DESIGN 4.16): the lists are drawn by the model's weights (set_negative_weights) and
        every sampled loss — a caller's `candidates` / `shared` too — subtracts log Q(c) from the label's and every slot's logit.
        FLAGS.sampled_loss other than "softmax" (DESIGN 4.19): binary cross-entropy or BPR over the same slots and values, for the
        model's own lists and a caller's alike; lists, log-Q, lazy_adam and deterministic are untouched by the objective."""
        tab = self.item_embs.lookup_table
        if candidates is not None and shared is not None:
            raise ValueError("_score_ce: both `candidates` and `shared` are given: one estimator per call")
        if shared is None and candidates is None and self.shared_negatives > 0:
            shared = self.draw_shared_negatives(labels.device)
        sampled = shared is not None or candidates is not None or self.train_negatives > 0
        # FLAGS.neg_sampler: a non-uniform sampler corrects every sampled loss by log Q, a caller's list included
        dist = self._negative_dist() if sampled else None
        tail = () if dist is None else (dist.logq_on(labels.device),)
        if sampled and self.sampled_loss != "softmax":
            tail = (None if dist is None else tail[0], self.sampled_loss)
            if candidates is None and shared is None:
                candidates = self._sample(None, labels, self.train_negatives, self.train_neg_seed, self.neg_step, 0, dist)
            if self.lazy_adam:
                self._lazy_lists = (labels, candidates, shared)
            fn, lists = (ops.SharedCEFn, shared) if shared is not None else (ops.SampledCEFn, candidates)
            return fn.apply(rows, tab, self.output_bias, self.compute(tab), labels, lists, self.deterministic,
                            self._lazy_grad if self.lazy_adam else None, *tail)
        if shared is not None:
            if self.lazy_adam:
                self._lazy_lists = (labels, None, shared)
            return ops.SharedCEFn.apply(rows, tab, self.output_bias, self.compute(tab), labels, shared, self.deterministic,
                                        self._lazy_grad if self.lazy_adam else None, *tail)
        if not sampled:
            return ops.ScoreCEFn.apply(rows, tab, self.output_bias, self.compute(tab), labels, self.deterministic)
        if candidates is None:
            candidates = self._sample(None, labels, self.train_negatives, self.train_neg_seed, self.neg_step, 0, dist)
        if self.lazy_adam:      # (the table gradient is added into the arena; the optimizer needs the step's lists)
            self._lazy_lists = (labels, candidates, None)
            return ops.SampledCEFn.apply(rows, tab, self.output_bias, self.compute(tab), labels, candidates, self.deterministic,
                                         self._lazy_grad, *tail)
        if dist is not None:
            return ops.SampledCEFn.apply(rows, tab, self.output_bias, self.compute(tab), labels, candidates, self.deterministic, None,
                                         *tail)
        return ops.SampledCEFn.apply(rows, tab, self.output_bias, self.compute(tab), labels, candidates, self.deterministic)

    def _sample(self, seen, labels, n, seed, step, row0, dist):
        """ops.sample_negatives over [1, _negatives_hi()): uniform, or by `dist` (ops.NegDist)."""
        if dist is None:
            return ops.sample_negatives(seen, labels, n, 1, self._negatives_hi(), seed, step, row0)
        return ops.sample_negatives(seen, labels, n, 1, self._negatives_hi(), seed, step, row0, dist=dist)

    def draw_shared_negatives(self, device, step=None):
        """int32 [S]: the shared list of step `step` (default: neg_step) — the device sampler asked for one row of S negatives,
        from the model's negative distribution (FLAGS.neg_sampler)."""
        one = torch.zeros(1, device=device, dtype=torch.int64)
        return self._sample(None, one, self.shared_negatives, self.train_neg_seed, self.neg_step if step is None else step, 0,
                            self._negative_dist()).reshape(-1)

    # ---- weighted negatives ---------------------------------------------------------------------
    def negative_dist(self, weights, T_reject=0) -> "ops.NegDist":
        """ops.build_neg_dist over the model's negative range [1, _negatives_hi()) from per-item weights (float [>= hi], indexed by
        item id; entries outside the range are ignored); logq is sized to the item table.  T_reject: the seen ids a row may reject
        besides its label (training: 0; evaluation: the sequence length)."""
        import numpy as np
        w = np.asarray(weights, dtype=np.float64).reshape(-1)
        hi, rows = self._negatives_hi(), int(self.item_embs.lookup_table.shape[0])
        if w.shape[0] < hi:
            raise ValueError(f"negative weights: {w.shape[0]} entries, one per item id of [0, {hi}) are needed")
        full = np.zeros(rows, dtype=np.float64)
        full[:hi] = w[:hi]
        return ops.build_neg_dist(full, 1, hi, T_reject)

    def set_negative_weights(self, weights) -> None:
        """The weights FLAGS.neg_sampler draws training negatives by (float [>= hi], indexed by item id): ops.neg_weights gives the
        presets — popularity from item counts, log_uniform from the ids' order.  None: back to no weights."""
        if self.neg_sampler == "uniform":
            raise ValueError("set_negative_weights: neg_sampler is 'uniform' (FLAGS.neg_sampler = popularity or log_uniform)")
        self._neg_dist = None if weights is None else self.negative_dist(weights, 0)

    def _negative_dist(self):
        """None for the uniform sampler, else the training distribution; log_uniform needs nothing but the range and is built here."""
        if self.neg_sampler == "uniform":
            return None
        if self._neg_dist is None:
            if self.neg_sampler != "log_uniform":
                raise ValueError(f"neg_sampler={self.neg_sampler!r}: no weights yet — call model.set_negative_weights(weights) before "
                                 "the first training step (ops.neg_weights('popularity', I, 1, hi, counts, alpha) from item counts)")
            hi = self._negatives_hi()
            self.set_negative_weights(ops.neg_weights("log_uniform", hi, 1, hi))
        return self._neg_dist

    def train_step(self, features, labels):
        """One optimizer step: forward, backward, TF-Adam.  Returns the loss tensor (device scalar).
        With FLAGS.lazy_adam the item table's gradient is consumed row by row by the optimizer: after the step the
        table's `.grad` (and its entry of tf_gradients()) reads ZERO, not the step's gradient."""
        self.settle_state()
        ops.rng_advance(self._rng_state)
        self.detach_grads()
        loss = self.train_loss(features, labels)
        loss.backward()
        self.collect_grads()
        self.mask_padded_grads()
        self.optimizer_step()
        if self.train_negatives > 0 or self.shared_negatives > 0:
            self.neg_step += 1
        return loss.detach()

    # ---- Sequential.eval (Base.py:150-207) -------------------------------------------------------------------
    @torch.no_grad()
    def eval_topk(self, features, mask_seen=True, K=100):
        logits = self.forward(features, False)
        return ops.mask_topk(logits, 0, features["seqs_i"] if mask_seen else None, K)

    @torch.no_grad()
    def eval_rank(self, features, labels, mask_seen=True):
        """int32 [B]: the label's place in the (logit desc, item id asc) order of the unseen catalogue (Base.py:150-201), counted on the
        materialised logits — no top-K list, the logits are left as they are."""
        logits = self.forward(features, False)
        return ops.rank_from_logits(logits, 0, features["seqs_i"] if mask_seen else None, self._last_labels(labels))

    # ---- evaluation on candidate lists: sampled negatives and re-ranking -------------------------------------
    def _last_rows(self, features):
        """[B, C] rows of the last position: what every evaluation scores."""
        out = self.encoder(features, False, self._last_pos(features["seqs_i"]))
        rows = out[0] if isinstance(out, tuple) else out
        return rows.reshape(-1, self.num_units).contiguous()

    def _negatives_hi(self) -> int:
        """Negatives are drawn from [1, hi): every item id (a model with a MASK row excludes it)."""
        return self.num_items

    @torch.no_grad()
    def score_candidates(self, features, candidates, mask_seen=True):
        """f32 [B, N]: the logits of each sequence's own candidate list (int32 [B, N]; -1 = empty slot) — re-ranking.  -inf at an
        empty slot and, with mask_seen, at the ids of the sequence's history.  The item table is read at the listed rows only."""
        tab = self.item_embs.lookup_table
        return ops.score_candidates(self._last_rows(features), self.compute(tab), self.output_bias, candidates,
                                    features["seqs_i"] if mask_seen else None)[0]

    @torch.no_grad()
    def eval_candidates(self, features, labels, candidates=None, num_negatives=100, mask_seen=True, seed=0, step=0, row0=0, dist=None):
        """int32 [B]: the label's place among its candidates in the (logit desc, item id asc) order.  `candidates` int32 [B, N], or
        None: `num_negatives` ids per sequence drawn from the catalogue by ops.sample_negatives(seed, step, row0) — never an id of
        the sequence's history and never the label, whatever mask_seen says; mask_seen decides whether seen ids of a caller's list
        and a seen label read -inf.  `dist` (ops.NegDist, e.g. negative_dist(weights, T_reject=sequence length)): the
        negatives are drawn by its weights — the popularity-sampled protocol; the ranking uses the raw logits, no log-Q term."""
        lab = self._last_labels(labels)
        seen = features["seqs_i"]
        if candidates is None:
            candidates = self._sample(seen, lab, num_negatives, seed, step, row0, dist)
        tab = self.item_embs.lookup_table
        return ops.score_candidates(self._last_rows(features), self.compute(tab), self.output_bias, candidates,
                                    seen if mask_seen else None, lab, want_scores=False)[2]

    def reset_metrics(self, ks=None):
        """`ks`: the cut-offs of the by-rank metrics (eval_step(by_rank=True)); default (10, 50, 100), at most 8."""
        dev = self._arena.device
        self._metrics = torch.zeros(6, device=dev, dtype=torch.float32)
        self._metric_count = 0
        self._rank_ks = tuple(int(k) for k in (ks or (10, 50, 100)))
        if not 1 <= len(self._rank_ks) <= 8:
            raise ValueError(f"reset_metrics: 1 to 8 cut-offs (got {self._rank_ks})")
        self._rank_ks_dev = torch.tensor(self._rank_ks, device=dev, dtype=torch.int32)
        self._rank_sums = torch.zeros(2 * len(self._rank_ks) + 1, device=dev, dtype=torch.float32)
        self._rank_count = 0

    @torch.no_grad()
    def eval_step(self, features, labels, mask_seen=True, by_rank=False, *, candidates=None, negatives=0, neg_seed=0, row0=0,
                  neg_dist=None):
        """`candidates` (int32 [B, N]) or `negatives` > 0: the label is ranked inside the list / among that many sampled negatives
        (eval_candidates; `row0` = index of the batch's first sequence in its split) and the step accumulates like a by-rank step.
        `neg_dist` (ops.NegDist): the sampled negatives are drawn by its weights instead of uniformly."""
        if self._metrics is None:
            self.reset_metrics()
        on_list = candidates is not None or negatives > 0
        if by_rank or on_list:
            if self._metric_count != self._rank_count:
                raise RuntimeError("eval_step: by-rank and top-K steps cannot share one accumulation (call reset_metrics)")
            rank = (self.eval_candidates(features, labels, candidates, negatives, mask_seen, neg_seed, 0, row0, neg_dist) if on_list
                    else self.eval_rank(features, labels, mask_seen))
            # (steps on lists add row by row: with `row0` a split gives the same sums whatever the batch size)
            ops.rank_metrics_from_rank(rank, self._rank_ks_dev, self._rank_sums, row_order=on_list)
            self._rank_count += labels.shape[0]
        else:
            if self._rank_count:
                raise RuntimeError("eval_step: by-rank and top-K steps cannot share one accumulation (call reset_metrics)")
            _, idx = self.eval_topk(features, mask_seen)
            ops.rank_metrics(idx, labels[:, -1].contiguous(), self._metrics)
        self._metric_count += labels.shape[0]

    def metrics(self) -> Dict[str, float]:
        if getattr(self, "_rank_count", 0):     # by-rank steps: H / N at the chosen cut-offs and the mean reciprocal rank
            vals = (self._rank_sums / self._rank_count).tolist()
            names = [f"H{k}" for k in self._rank_ks] + [f"N{k}" for k in self._rank_ks] + ["MRR"]
            return dict(zip(names, vals))
        vals = (self._metrics / max(1, self._metric_count)).tolist()
        return dict(zip(("H10", "H50", "H100", "N10", "N50", "N100"), vals))
