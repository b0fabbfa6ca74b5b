"""Mirror of src/model/EasyDGL.py — same constructor / call surface, HIP kernels underneath.

    m = EasyDGL(num_items, FLAGS).finalize("cuda")
    logits = m(features, is_training)                 # EasyDGL.__call__  (EasyDGL.py:69-151)
    loss   = m.train_loss(features, labels)           # the scalar EasyDGL.train minimises (:153-188)
    loss   = m.train_step(features, labels)           # + backward + Adam (the reference's train_op)
    m.eval_step(features, labels, mask_seen=True)     # Sequential.eval (Base.py:150-207) accumulators

``features``: dict with ``seqs_i`` int64 [B,T], ``seqs_t`` float32 [B,T] (seconds), ``masked_positions``
int64 [B,M] (training only) — exactly what MAUPostProcessor emits (dataloader.py:159-206).
"""
from __future__ import annotations

import pickle
from typing import Dict

import numpy as np
import torch
from torch import nn

from .. import ops
from ..module import coding as C
from ..module import temporal as T
from .base import Sequential, _Dense, _LayerNorm  # noqa: F401  (the parameter holders are imported from here elsewhere)


class _Block(nn.Module):
    def __init__(self, cin, C_, heads, events, att_drop, gen):
        super().__init__()
        self.attention = T.BiMAU(C_, heads, events, att_drop, in_units=cin, gen=gen)   # layer_i/attention/self/TMAU
        self.att_out = _Dense(C_, C_, gen)                                 # layer_i/attention/output/dense
        self.att_ln = _LayerNorm(C_)                                       # layer_i/attention/output/LayerNorm
        self.inter = _Dense(C_, 2 * C_, gen)                               # layer_i/intermediate/dense
        self.out = _Dense(2 * C_, C_, gen)                                 # layer_i/output/dense
        self.out_ln = _LayerNorm(C_)                                       # layer_i/output/LayerNorm


class EasyDGL(Sequential):
    tf_numpy = False     # tf_values() / tf_gradients(): torch tensors on the parameters' device
    lazy_adam_ok = True  # (edgl_encode_bwd_add_* ADD the item gradient into d_item)

    def __init__(self, num_items, FLAGS):
        super().__init__(num_items, FLAGS)
        self.mask = num_items            # EasyDGL.py:39
        self.seqslen += 1                # EasyDGL.py:40
        self.num_items += 1              # EasyDGL.py:41
        self.masklen = FLAGS.masklen
        self.time_scale = float(FLAGS.time_scale)
        self.seed = int(getattr(FLAGS, "seed", 9876))
        table = getattr(FLAGS, "mark_table", None)
        if table is None:
            table = pickle.load(open(FLAGS.mark, "rb")).toarray()   # EasyDGL.py:45
        table = np.asarray(table)
        if table.shape[0] < num_items:
            raise ValueError("mark table needs one row per item id < num_items")
        if not np.isin(table, (0, 1)).all():
            raise ValueError("mark table must be 0/1 multi-hot")
        self.num_events = int(table.shape[-1])                     # EasyDGL.py:46
        if not (2 <= self.num_events <= T.MAX_EVENTS):
            raise ValueError(f"num_events must be in [2, {T.MAX_EVENTS}] (more than 16 run as mark groups: temporal.modulated_attention)")
        self.register_buffer("mark_lookup_table", torch.from_numpy(table.astype(np.uint8)), persistent=False)
        self.ct_reg = float(getattr(FLAGS, "ct_reg", 0.0) or 0.0)

        gen = torch.Generator().manual_seed(self.seed)
        # A head dim the attention kernels do not tile runs zero-padded at the next of 16 / 32 / 64 / 128 (model/base.py: channel
        # padding); here only even head dims (the time code pairs channels), and nothing above the largest kernel.  The one
        # gradient that is not zero on a padded entry by itself is masked in mask_padded_grads.
        H = self.num_heads
        dh = self.num_units // H if H > 0 and self.num_units % H == 0 else 0
        if dh and dh not in T.SUPPORTED_HEAD_DIMS and (dh % 2 or dh > T.SUPPORTED_HEAD_DIMS[-1]):
            raise ValueError(f"EasyDGL: head dim num_units/num_heads = {dh}: even head dims up to {T.SUPPORTED_HEAD_DIMS[-1]} "
                             "run (zero-padded to the next of 16 / 32 / 64 / 128)")
        self._setup_channel_pad("EasyDGL")
        C_ = self.num_units
        # variable scope "CSTMA" (EasyDGL.py:49-57)
        self.item_embs = C.Embedding(self.num_items, C_, self.l2_reg, zero_pad=True, scale=True, gen=gen)
        self.mark_embs = C.Embedding(self.num_events, C_, self.l2_reg, zero_pad=True, scale=False, gen=gen)
        self.pcoding = C.PositionCoding(self.seqslen, C_, self.l2_reg, gen=gen)
        self.tcoding = C.TimeSinusoidCoding(C_)
        self.output_bias = self.make_output_bias()
        self.layers = nn.ModuleList()
        for i in range(FLAGS.num_blocks):
            self.layers.append(_Block(3 * C_ if i == 0 else C_, C_, self.num_heads, self.num_events,
                                      self.attention_probs_dropout_rate, gen))
        if FLAGS.num_blocks == 0 and self.pad[0]:
            raise ValueError("EasyDGL: --num_blocks 0 with a channel-padded width is not supported (the head transform would read the "
                             "padded 3C-wide encoder output)")
        # (no block: the head transform reads the 3C-wide encoder output — tf.layers.dense builds its kernel from the input width,
        #  EasyDGL.py:138)
        self.transform = _Dense(3 * C_ if FLAGS.num_blocks == 0 else C_, C_, gen)       # cls/predictions/transform/dense
        self.transform_ln = _LayerNorm(C_)         # cls/predictions/transform/LayerNorm
        self._finish_pad(gen)

    # ---- the variable table (model/base.py derives load / values / gradients / the padded storage from it) ----------------------
    def _pad_specs(self):
        """(TF name, parameter, axis maps reference -> stored (None = axis kept), initialiser of the TRUE-shape variable)."""
        c, c3, c4 = self._cmap(), self._cmap(3), self._cmap(4)
        h2 = torch.arange(2 * self.width_true)
        st_rows, j, u = self._mlp_maps()
        tr = self.transform
        sp = [("CSTMA/item_embs/lookup_table", self.item_embs.lookup_table, (None, c), "glorot"),
              ("CSTMA/mark_embs/lookup_table", self.mark_embs.lookup_table, (None, c), "glorot"),
              ("CSTMA/spatial_embs/embedding/lookup_table", self.pcoding.pembs.lookup_table, (None, c), "glorot"),
              ("CSTMA/output_bias", self.output_bias, (None,), "zeros"),
              ("cls/predictions/transform/dense/kernel", tr.kernel, (c if self.layers else c3, c), "glorot"),   # (no block: 3C rows)
              ("cls/predictions/transform/dense/bias", tr.bias, (c,), "zeros"),
              ("cls/predictions/transform/LayerNorm/beta", self.transform_ln.beta, (c,), "zeros"),
              ("cls/predictions/transform/LayerNorm/gamma", self.transform_ln.gamma, (c,), "ones")]
        for i, blk in enumerate(self.layers):
            pre = f"layer_{i}/"
            tm = pre + "attention/self/TMAU/"
            st = tm + "sequential_temporal_combined/"
            a = blk.attention
            sp += [(tm + "dense/kernel", a.dense_kernel, (c3 if i == 0 else c, c4), "normal"),
                   (tm + "dense/bias", a.dense_bias, (c4,), "zeros"),
                   (st + "dense/kernel", a.st_kernel, (st_rows, j), "glorot"),
                   (st + "dense/bias", a.st_bias, (j,), "zeros"),
                   (st + "weight", a.weight, (None, u), "glorot"),
                   (st + "scaling", a.scaling, (None,), "zeros"),
                   (pre + "attention/output/dense/kernel", blk.att_out.kernel, (c, c), "glorot"),
                   (pre + "attention/output/dense/bias", blk.att_out.bias, (c,), "zeros"),
                   (pre + "attention/output/LayerNorm/beta", blk.att_ln.beta, (c,), "zeros"),
                   (pre + "attention/output/LayerNorm/gamma", blk.att_ln.gamma, (c,), "ones"),
                   (pre + "intermediate/dense/kernel", blk.inter.kernel, (c, h2), "glorot"),
                   (pre + "intermediate/dense/bias", blk.inter.bias, (h2,), "zeros"),
                   (pre + "output/dense/kernel", blk.out.kernel, (h2, c), "glorot"),
                   (pre + "output/dense/bias", blk.out.bias, (c,), "zeros"),
                   (pre + "output/LayerNorm/beta", blk.out_ln.beta, (c,), "zeros"),
                   (pre + "output/LayerNorm/gamma", blk.out_ln.gamma, (c,), "ones")]
        return sp

    def tf_variable_map(self) -> Dict[str, nn.Parameter]:
        """Reference variable name (scope main/...) -> parameter (each parameter is one variable here)."""
        return {name: p for name, p, _, _ in self._pad_specs()}

    @torch.no_grad()
    def _init_padded(self, gen):
        """The base initialisers (temporal.py:393 N(0, 0.02) among them), then the time-code scales of the TRUE width
        (coding.py:132-136)."""
        super()._init_padded(gen)
        dhp, dht = self.pad
        Ct, Cp = self.width_true, self.num_units
        true_scale = np.power(10000, np.arange(0, Ct, 2) * 1.0 / Ct).astype(np.float32)      # pair j of the TRUE channels
        sc = np.ones(Cp // 2, np.float32)
        for c in range(0, Ct, 2):
            cp = (c // dht) * dhp + (c % dht)
            sc[cp // 2] = true_scale[c // 2]
        self.tcoding.scale = torch.from_numpy(sc).to(self.tcoding.scale.device)

    def mask_padded_grads(self) -> None:
        """The one gradient that is not zero on a padded entry by itself: the intensity MLP's output weights w[e, u >= dh_true]
        (their hidden units sit at sigmoid(0) = 1/2 and collect d z).  Zeroed before the optimizer sees them."""
        if not self.pad[0]:
            return
        for blk in self.layers:
            g = blk.attention.weight.grad
            if g is not None:
                g[:, self.pad[1]:].zero_()

    def l2_param_names(self):
        return ["item_embs.lookup_table", "mark_embs.lookup_table", "pcoding.pembs.lookup_table"]

    def encode(self, features, is_training):
        """EasyDGL.py:70-95 -> (X0 [B,T,3C], spans [B,T], marks [B,T,E] uint8)."""
        ids, ts = features["seqs_i"], features["seqs_t"]
        tab = self.item_embs.lookup_table
        return ops.EncodeFn.apply(tab, self.pcoding.pembs.lookup_table, self.mark_embs.lookup_table, self.compute(tab),
                                  ids, ts, self.mark_lookup_table, self.tcoding.scale, self.mask, self.time_scale,
                                  self._drop(self.hidden_dropout_rate, 1, is_training), self.act_dtype, self.pad,
                                  self.deterministic, self._lazy_grad if (self.lazy_adam and is_training) else None)

    def encoder(self, features, is_training, gather_pos):
        """EasyDGL.py:70-146: returns (rows [B*Mg, C] at gather_pos, [lambda per block])."""
        ids = features["seqs_i"]
        C_ = self.num_units
        x, spans, marks = self.encode(features, is_training)
        lams = []
        fused_eval = self._eval_tail_ok(is_training, x, gather_pos)
        for i, blk in enumerate(self.layers):
            layer_in = x
            att, lam = blk.attention(layer_in, layer_in, ids, spans, marks, is_training,
                                     drop=self._drop(self.attention_probs_dropout_rate, 10 + 4 * i, is_training))
            lams.append(lam)
            if fused_eval:      # inference: the block tail (and the head behind the last block) as ONE launch (csrc/k_tail_fwd.hip)
                last = i == len(self.layers) - 1
                x, rows = self._eval_tail(blk, att.contiguous(), layer_in, gather_pos, last)
                if last:
                    return rows, lams
                continue
            att = self._linear(att, blk.att_out)                                                   # :113
            att = ops.AddLayerNormFn.apply(att, layer_in[:, :, :C_], blk.att_ln.gamma, blk.att_ln.beta,
                                           self._drop(self.hidden_dropout_rate, 11 + 4 * i, is_training), None, self.pad)  # :114-116
            inter = self._linear(att, blk.inter, True)                                        # :120-121
            out = self._linear(inter, blk.out)                                                     # :125
            x = ops.AddLayerNormFn.apply(out, att, blk.out_ln.gamma, blk.out_ln.beta,
                                         self._drop(self.hidden_dropout_rate, 12 + 4 * i, is_training), None, self.pad)   # :126-128
        so = self._linear(x, self.transform, True)                                           # :138
        rows = ops.AddLayerNormFn.apply(so, None, self.transform_ln.gamma, self.transform_ln.beta, ops.NO_DROP,
                                        gather_pos, self.pad)                                      # :139,142-146
        return rows, lams

    # ---- inference through the fused block tail (the training engine's forward kernel; EasyDGL.py:110-146) ---------------------
    def _eval_tail_ok(self, is_training, x, gather_pos) -> bool:
        import os
        from .. import _lib
        if is_training or torch.is_grad_enabled() or not self.layers or x.dtype != torch.bfloat16:
            return False
        if os.environ.get("EDGL_EVAL_FUSED_TAIL", "1") == "0" or gather_pos.shape[1] > 256:
            return False
        return bool(_lib.lib.edgl_tail_supported(x.shape[1], self.num_units, _lib.BF16))

    def _eval_tail(self, blk, att, layer_in, gather_pos, last):
        """One block tail in one launch: att_out dense -> +residual -> LN1 -> inner dense + GELU -> out dense -> +residual -> LN2
        (-> head transform + GELU + LN3 + row gather behind the last block).  The tensors the kernel saves for a backward go to
        a scratch set kept per (batch, length); dropout rate 0.  Returns (y [B, T, C], head rows [B*Mg, C] or None)."""
        from .. import _lib
        lib, P = _lib.lib, ops._ptr
        B, T, C = att.shape
        Mg = gather_pos.shape[1]
        dev, dt = att.device, att.dtype
        key = (B, T, Mg, str(dev))
        ws = getattr(self, "_eval_tail_ws", None)
        if ws is None or ws["key"] != key:
            e = lambda *sh, d=dt: torch.empty(sh, device=dev, dtype=d)  # noqa: E731
            ws = dict(key=key, pack=e(int(lib.edgl_tail_pack_elems(C))), ao=e(B, T, C), a1=e(B, T, C), pre_f=e(B, T, 2 * C),
                      f=e(B, T, 2 * C), o=e(B, T, C), pre_t=e(B, T, C), so=e(B, T, C), st1=e(B, 2, d=torch.float32),
                      st2=e(B, 2, d=torch.float32), st3=e(B, 2, d=torch.float32))
            self._eval_tail_ws = ws
        st = ops._stream()
        _lib.check(lib.edgl_tail_pack(P(self.compute(blk.att_out.kernel)), P(self.compute(blk.inter.kernel)),
                                      P(self.compute(blk.out.kernel)), P(self.compute(self.transform.kernel)), C, P(ws["pack"]), st),
                   "edgl_tail_pack")
        y = torch.empty((B, T, C), device=dev, dtype=dt)
        rows = torch.empty((B * Mg, C), device=dev, dtype=dt) if last else None
        tl = self.transform_ln
        _lib.check(lib.edgl_tail_fwd_ct(P(att), layer_in.data_ptr(), layer_in.shape[2], P(ws["pack"]), P(blk.att_out.bias),
                                     P(blk.inter.bias), P(blk.out.bias), P(self.transform.bias), P(blk.att_ln.gamma),
                                     P(blk.att_ln.beta), P(blk.out_ln.gamma), P(blk.out_ln.beta), P(tl.gamma), P(tl.beta), B, T, C,
                                     0.0, None, 0, 0, P(gather_pos), Mg, int(last), P(ws["ao"]), P(ws["a1"]), P(ws["st1"]),
                                     P(ws["pre_f"]), P(ws["f"]), P(ws["o"]), P(y), P(ws["st2"]), P(ws["pre_t"]), P(ws["so"]),
                                     P(ws["st3"]), P(rows), None, self.pad[0], self.pad[1], _lib.BF16, st), "edgl_tail_fwd")
        return y, rows

    def _gather_pos(self, features, is_training):
        return features["masked_positions"].contiguous() if is_training else self._last_pos(features["seqs_i"])

    def _last_rows(self, features):
        return self.encoder(features, False, self._gather_pos(features, False))[0].contiguous()

    def _negatives_hi(self) -> int:
        return self.mask      # (the MASK row is not an item)

    # ---- EasyDGL.__call__ ------------------------------------------------------------------------------
    def forward(self, features: Dict[str, torch.Tensor], is_training: bool):
        """Returns logits [B*M, I] (training) / [B, I] (eval), materialised like the reference (:149-151)."""
        rows, lams = self.encoder(features, is_training, self._gather_pos(features, is_training))
        self._last_lams = lams
        tab = self.item_embs.lookup_table
        return ops.ScoreLogitsFn.apply(rows, tab, self.output_bias, self.compute(tab))

    # ---- EasyDGL.train (the loss it builds) ------------------------------------------------------------------
    def train_loss(self, features, labels, *, candidates=None, shared=None):
        """EasyDGL.py:153-188 with the fused scoring/CE path (no [B*M, I] tensor).  `candidates` (int32 [B*M, N]) or
        FLAGS.train_negatives > 0: the softmax of every masked position over its label and its own list (Sequential._score_ce).
        FLAGS.lazy_adam: the backward of this loss ADDS the item table's gradient into the table's view of the
        gradient arena (no dense [I, C] temporary), and the call's (seqs_i, labels, candidates) are remembered for the optimizer
        step, which walks only those rows.  The item table's l2 term still enters the loss (the value stays comparable with the
        dense mode) but its backward returns no dense tensor: l2_reg * w reaches the table inside edgl_adam_rows, so only touched
        rows decay.  The mark and position tables keep the dense l2 gradient.
        `shared` (int32 [S]) or FLAGS.shared_negatives > 0: every masked position against its label and the step's ONE
        list; lazy_adam then remembers (seqs_i and the list, labels): a live slot of the list is touched whenever the step ran."""
        rows, lams = self.encoder(features, True, self._gather_pos(features, True))
        loss = self._score_ce(rows, labels.reshape(-1).contiguous(), candidates, shared)
        if self.lazy_adam and torch.is_grad_enabled():
            lab, cand, sh = self._lazy_lists
            ids = features["seqs_i"] if sh is None else torch.cat((features["seqs_i"].reshape(-1), sh.long()))
            self._lazy_pending.append((ids, lab, cand))
        if self.l2_reg != 0.0:                                                                     # :158
            loss = loss + ops.L2Fn.apply(self.item_embs.lookup_table, self.l2_reg, self.lazy_adam)
            for p in (self.mark_embs.lookup_table, self.pcoding.pembs.lookup_table):
                loss = loss + ops.L2Fn.apply(p, self.l2_reg)
        if self.ct_reg != 0.0:                                                                     # :159-175
            for lam in lams:
                loss = loss + ops.TppFn.apply(lam, features["masked_positions"].contiguous(), labels.contiguous(),
                                              features["seqs_t"], self.mark_lookup_table, self.num_heads,
                                              self.ct_reg / self.num_heads)
        return loss

    # ---- Sequential.eval (Base.py:150-207) ----------------------------------------------------------------
    @torch.no_grad()
    def eval_topk(self, features, mask_seen=True, K=100):
        rows, _ = self.encoder(features, False, self._gather_pos(features, False))
        tab = self.item_embs.lookup_table
        return ops.score_topk(rows, self.compute(tab), self.output_bias, features["seqs_i"] if mask_seen else None, K, 0,
                              self.num_items)

    @torch.no_grad()
    def eval_topk_sharded(self, features, mask_seen=True, K=100, group=None, world=None, rank=None):
        """Row-sharded full-catalogue scoring: this rank scores the batch against its contiguous
        shard of the item table, masks seen ids that fall in the shard, keeps a local top-K with GLOBAL ids; one
        packed all-gather + merge kernel give the global top-K.  `world`/`rank` may be passed explicitly to
        emulate S shards in one process (tests); with torch.distributed they come from the process group."""
        from .. import parallel
        rows, _ = self.encoder(features, False, self._gather_pos(features, False))
        tab_c = self.compute(self.item_embs.lookup_table)
        seen = features["seqs_i"] if mask_seen else None

        def local_topk(i0, i1):
            if i1 <= i0:
                R = rows.shape[0]
                return (torch.full((R, K), float("-inf"), device=rows.device),
                        torch.full((R, K), -1, device=rows.device, dtype=torch.int32))
            return ops.score_topk(rows, tab_c, self.output_bias, seen, K, i0, i1)

        if world is not None:   # in-process emulation of `world` shards
            vals, idxs = zip(*(local_topk(*parallel.shard_bounds(self.num_items, world, r)) for r in range(world)))
            return ops.topk_merge(torch.stack(vals), torch.stack(idxs))
        return parallel.sharded_topk(local_topk, ops.topk_merge, self.num_items, K, group)

    @torch.no_grad()
    def eval_rank(self, features, labels, mask_seen=True):
        """int32 [B]: the place of each sequence's true next item in the (logit desc, item id asc) order of the unseen catalogue
        (Base.py:150-201) by one counting sweep — no top-K list (ops.score_label_rank)."""
        rows, _ = self.encoder(features, False, self._gather_pos(features, False))
        tab = self.item_embs.lookup_table
        return ops.score_label_rank(rows, self.compute(tab), self.output_bias, features["seqs_i"] if mask_seen else None,
                                    self._last_labels(labels), 0, self.num_items)

    @torch.no_grad()
    def eval_rank_sharded(self, features, labels, mask_seen=True, group=None, world=None, rank=None):
        """eval_rank with the item table row-sharded: this rank counts over its parallel.shard_bounds range and ONE all-reduce (SUM)
        of the int32 [B] counts gives the ranks — no candidate lists, no merge; an empty shard contributes zeros.  `world` emulates
        the shards in one process (tests), as eval_topk_sharded does."""
        from .. import parallel
        rows, _ = self.encoder(features, False, self._gather_pos(features, False))
        tab_c = self.compute(self.item_embs.lookup_table)
        seen = features["seqs_i"] if mask_seen else None
        lab = self._last_labels(labels)

        def count_local(i0, i1):
            return ops.score_label_rank(rows, tab_c, self.output_bias, seen, lab, i0, i1)

        if world is not None:   # in-process emulation of `world` shards
            return sum(count_local(*parallel.shard_bounds(self.num_items, world, r)) for r in range(world))
        return parallel.sharded_rank(count_local, self.num_items, group)
