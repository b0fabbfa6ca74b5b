"""Train / evaluate driver — the role of the reference's ``src/main.py:78-151`` with ``util.EarlyStopping``
(``src/util.py:14-58``), on the HIP model.

Models: EasyDGL (masked batches, ``MAUPostProcessor``) and CTSMA / TGAT / TiSASREC / SASREC / S2PNM (regressive batches,
``RegressivePostProcessor``), chosen as ``util.reader`` does (``util.py:99-129``); TimelyREC is fed regressively with the four
calendar fields of its records (``has_datetime=True``), derived from ``seqs_t`` where the files lack them.
Same flags as ``main.py:22-75`` for everything these paths read (``--train/--valid/--test`` file patterns,
``--num_items --num_units --num_heads --num_blocks --seqslen --time_scale --masklen --mark --ct_reg --batch_size
--num_epochs --learning_rate --l2_reg --hidden_dropout_rate --attention_probs_dropout_rate --eval_per_steps
--mask_seen``).  Epoch structure as in the reference: one pass over the training records (masked on the device, one
kernel per batch), then validation and test passes with the last position masked, model selection on validation H@100,
patience 10, stop on a NaN loss, best checkpoint kept.  Differences, stated: records are shuffled with a full
permutation per epoch (the reference: file-order shuffle + a 64-record buffer, ``dataloader.py:222-236``); full batches
run through the static ``TrainEngine`` and the remainder batch through ``model.train_step``.  ``--device_data`` keeps the
three splits in device memory and assembles the same batches there (``data.DeviceLoader``); with ``--graph`` the
EasyDGL step is then replayed as one HIP graph.

``python -m easydgl_amd.train --model EasyDGL --train 'data/train*.tfrec' --valid data/validation.tfrec
--test data/test.tfrec --num_items 17770 --mark data/mark.pkl ...`` (``.npz`` files from ``formats.convert`` work too).
"""
from __future__ import annotations

import argparse
import logging
import math
import os
from types import SimpleNamespace
from typing import Dict, Optional

import numpy as np


def args(argv=None):
    p = argparse.ArgumentParser(description="EasyDGL (self-modulating attention) on MI355X — train / evaluate")
    p.add_argument("--train", required=True, help="training data file patterns (.tfrec or .npz)")
    p.add_argument("--valid", required=True)
    p.add_argument("--test", required=True)
    p.add_argument("--model", required=True, help="algorithm name: EasyDGL, CTSMA, TGAT, TiSASREC, SASREC, S2PNM or TimelyREC (util.ranking keys)")
    p.add_argument("--num_items", type=int, required=True)
    # reference default: 50 (main.py:35) — head dim 50 with the default single head: every model runs it zero-padded at head dim 64
    # (model/base.py, model/easydgl.py: exact, the padded channels stay zero); every published recipe passes --num_units=512
    # (runme.sh:15-115)
    p.add_argument("--num_units", type=int, default=50)
    p.add_argument("--num_heads", type=int, default=1)
    p.add_argument("--num_blocks", type=int, default=3)
    p.add_argument("--seqslen", type=int, default=30)
    p.add_argument("--time_scale", type=float, default=1)
    p.add_argument("--window_ratio", type=float, default=0.2,
                   help="TimelyREC: the calendar-slot window of a granularity is max(int(range * window_ratio + 0.5), 1) + 1; in (0, 0.5]")
    p.add_argument("--masklen", type=int, default=6)
    p.add_argument("--timelen", type=int, default=256)
    p.add_argument("--mark", type=str, help="mark data file (pickled csr matrix or .npy)")
    p.add_argument("--ct_reg", type=float, default=0.0)
    p.add_argument("--batch_size", type=int, default=128)
    p.add_argument("--num_epochs", type=int, default=100)
    p.add_argument("--learning_rate", type=float, default=5e-4)
    p.add_argument("--l2_reg", type=float, default=0.0)
    p.add_argument("--hidden_dropout_rate", type=float, default=0.0)
    p.add_argument("--attention_probs_dropout_rate", type=float, default=0.0)
    p.add_argument("--eval_per_steps", type=int, default=1)
    p.add_argument("--mask_seen", action="store_true")
    # build-specific
    p.add_argument("--dtype", choices=["bf16", "f32"], default="bf16", help="activation dtype of the HIP kernels")
    p.add_argument("--ckpt_dir", default="ckpt")
    p.add_argument("--seed", type=int, default=9876)   # main.py:156-159
    p.add_argument("--patience", type=int, default=10)
    p.add_argument("--graph", action="store_true",
                   help="regressive models: replay the training step of full batches as one HIP graph (Sequential.graphed_train_step); "
                        "with --device_data also EasyDGL: the engine's step is captured together with the on-device batch loader")
    p.add_argument("--device_data", action="store_true",
                   help="keep the train / valid / test splits in device memory and assemble every batch there (data.DeviceLoader): no "
                        "host indexing and no host-to-device copy per step; refused when the splits do not fit in free device memory")
    p.add_argument("--deterministic", action="store_true",
                   help="EasyDGL: bitwise reproducible training (main.py:157-168 pins TF_DETERMINISTIC_OPS): the item-table gradient "
                        "as ordered sums instead of f32 atomics, in the engine and in train_step")
    p.add_argument("--eval_by_rank", action="store_true",
                   help="evaluate by the label's rank (one counting sweep over the item table, ops.score_label_rank) instead of a top-K "
                        "list; same H / N metrics plus MRR")
    p.add_argument("--eval_negatives", type=int, default=0,
                   help="N > 0: the sampled-negative protocol — rank the true next item among N items drawn from the catalogue that the "
                        "user has not interacted with (ops.sample_negatives; the same N for every epoch), report H / N at 1, 5, 10 and "
                        "MRR, select the model on H10.  0: rank against the whole catalogue")
    p.add_argument("--eval_neg_seed", type=int, default=0, help="seed of the sampled negatives")
    p.add_argument("--train_negatives", type=int, default=0,
                   help="N > 0: sampled-softmax training (DESIGN 4.13) — the cross-entropy of every scored position over its label and N "
                        "negatives drawn uniformly from the catalogue (fresh lists every step) instead of the whole catalogue; every "
                        "batch goes through model.train_step (no static engine, no --graph).  0: full softmax")
    p.add_argument("--shared_negatives", type=int, default=0,
                   help="S > 0: sampled-softmax training on ONE list of S negatives per step, shared by every scored position (DESIGN "
                        "4.15; tf.nn.sampled_softmax_loss's default form) — scoring and gradients run as dense products on the matrix "
                        "pipe; a different estimator from --train_negatives, not both; no static engine, no --graph.  0: off")
    p.add_argument("--train_neg_seed", type=int, default=0, help="seed of the sampled training negatives")
    p.add_argument("--lazy_adam", action="store_true",
                   help="EasyDGL with --train_negatives or --shared_negatives: lazy row-wise Adam for the item table (DESIGN 4.14, TensorFlow's "
                        "LazyAdamOptimizer) — the table gradient lands in place and the optimizer updates only the rows the step used "
                        "(input ids, labels, negatives); every other parameter keeps the dense Adam")
    p.add_argument("--neg_sampler", choices=("uniform", "popularity", "log_uniform"), default="uniform",
                   help="with --train_negatives / --shared_negatives: the distribution the training negatives are drawn from (DESIGN "
                        "4.16).  popularity: (count + 1)^neg_alpha over the item counts of the training split; log_uniform: "
                        "TensorFlow's default, for ids sorted by falling frequency.  Both subtract log Q(c) from every sampled logit")
    p.add_argument("--neg_alpha", type=float, default=0.75, help="exponent of the popularity sampler (word2vec: 0.75)")
    p.add_argument("--sampled_loss", choices=("softmax", "bce", "bpr"), default="softmax",
                   help="with --train_negatives / --shared_negatives: the objective over the sampled negatives (DESIGN 4.19).  bce: "
                        "binary cross-entropy, the negatives summed (SASRec / TiSASRec / TGAT as published; with a weighted sampler, "
                        "tf.nn.nce_loss without its constant); bpr: the pairwise loss, averaged over a position's negatives")
    p.add_argument("--eval_neg_sampler", choices=("uniform", "popularity"), default="uniform",
                   help="with --eval_negatives: draw the evaluation negatives by (count + 1)^neg_alpha over the training split's item "
                        "counts — the popularity-sampled protocol; ranking uses the raw logits")
    a = p.parse_args(argv)
    if a.neg_sampler != "uniform" and a.train_negatives <= 0 and a.shared_negatives <= 0:
        p.error("--neg_sampler needs --train_negatives N > 0 or --shared_negatives S > 0: the full softmax draws no negatives")
    if a.sampled_loss != "softmax" and a.train_negatives <= 0 and a.shared_negatives <= 0:
        p.error("--sampled_loss needs --train_negatives N > 0 or --shared_negatives S > 0: the objective is defined over sampled negatives")
    if a.eval_neg_sampler != "uniform" and a.eval_negatives <= 0:
        p.error("--eval_neg_sampler needs --eval_negatives N > 0")
    if a.train_negatives > 0 and a.shared_negatives > 0:
        p.error("--shared_negatives with --train_negatives: one estimator per run (per-row lists or one shared list)")
    if a.shared_negatives < 0 or a.shared_negatives > 8192:
        p.error("--shared_negatives: the length of the step's shared negative list (0: off, at most 8192)")
    if a.shared_negatives > 0 and a.graph:
        p.error("--graph with --shared_negatives: the sampled-softmax step runs on the autograd path (model.train_step), whose "
                "negative lists are keyed by a host-side step count; it is not captured into a graph")
    if a.lazy_adam and a.train_negatives <= 0 and a.shared_negatives <= 0:
        p.error("--lazy_adam needs --train_negatives N > 0 or --shared_negatives S > 0: the full softmax has a dense table gradient, there are no untouched rows")
    if a.train_negatives < 0:
        p.error("--train_negatives: the number of sampled negatives per position (0: full softmax)")
    if a.train_negatives > 0 and a.graph:
        p.error("--graph with --train_negatives: the sampled-softmax step runs on the autograd path (model.train_step), whose "
                "negative lists are keyed by a host-side step count; it is not captured into a graph")
    return a


class EarlyStopping:
    """``util.EarlyStopping`` (util.py:14-58), decision for decision: the first evaluation sets the reference point; an
    evaluation with ``acc < best_acc`` increments the counter (stop at ``patience``); otherwise the counter resets, the
    checkpoint is saved and every test metric whose validation value did not fall below the FIRST evaluation's value is
    refreshed (``best_valid`` is never updated in the reference — SURVEY Appendix B item 11 — kept as is).  NaN loss stops."""

    def __init__(self, model_name: str, patience: int = 10, saver=None):
        self.model = model_name
        self.patience = patience
        self.counter = 0
        self.res: Optional[Dict[str, float]] = None
        self.best_valid: Optional[Dict[str, float]] = None
        self.best_acc = None
        self.best_loss = None
        self.early_stop = False
        self.saver = saver

    def step(self, loss: float, acc: float, valid: Dict[str, float], test: Dict[str, float]) -> bool:
        if np.isnan(loss):
            self.early_stop = True
        elif self.best_loss is None:
            self.best_acc, self.best_loss = acc, loss
            self.best_valid, self.res = dict(valid), dict(test)
        elif acc < self.best_acc:
            self.counter += 1
            logging.info("EarlyStopping %s counter: %d out of %d", self.model, self.counter, self.patience)
            if self.counter >= self.patience:
                self.early_stop = True
        else:
            self.best_loss = min(loss, self.best_loss)
            self.best_acc = max(acc, self.best_acc)
            for k in self.res:
                if self.best_valid[k] <= valid[k]:
                    self.res[k] = test[k]
            self.counter = 0
            if self.saver is not None:
                self.saver()
        return self.early_stop

    def summary(self) -> Dict[str, float]:
        logging.info("SUMMARY: %s", {k: "{0:.5f}".format(v) for k, v in (self.res or {}).items()})
        return dict(self.res or {})


def save_checkpoint(model, path: str) -> None:
    """Parameters (flat f32 arena), Adam moments and step — everything a resumed run needs."""
    import torch
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    model.settle_state()       # (the static engine keeps the counters one step ahead: the file holds "steps taken")
    torch.save({"arena": model._arena.detach().cpu(), "adam_m": model._adam_m.cpu(), "adam_v": model._adam_v.cpu(),
                "adam_state": model._adam_state.cpu(), "rng_state": model._rng_state.cpu(),
                "offsets": dict(model._offsets), "neg_step": int(getattr(model, "neg_step", 0)),
                "neg_sampler": str(getattr(model, "neg_sampler", "uniform")), "neg_alpha": float(getattr(model, "neg_alpha", 0.75)),
                "sampled_loss": str(getattr(model, "sampled_loss", "softmax"))},
               path)


def load_checkpoint(model, path: str) -> None:
    import torch
    ck = torch.load(path, map_location="cpu")
    if dict(ck["offsets"]) != dict(model._offsets):
        raise ValueError("checkpoint does not match the model's parameter layout")
    # (optional fields, DESIGN 4.16: a resumed run must draw the lists the uninterrupted run would have drawn)
    saved = (str(ck.get("neg_sampler", "uniform")), float(ck.get("neg_alpha", 0.75)))
    mine = (str(getattr(model, "neg_sampler", "uniform")), float(getattr(model, "neg_alpha", 0.75)))
    if saved[0] != mine[0] or (saved[0] == "popularity" and saved[1] != mine[1]):
        raise ValueError(f"checkpoint was trained with neg_sampler={saved[0]!r} neg_alpha={saved[1]}, the model has "
                         f"neg_sampler={mine[0]!r} neg_alpha={mine[1]}: a resumed run keeps its negative sampler")
    # (optional field, DESIGN 4.19: a file from before it existed was trained with the softmax)
    saved_loss, my_loss = str(ck.get("sampled_loss", "softmax")), str(getattr(model, "sampled_loss", "softmax"))
    if saved_loss != my_loss:
        raise ValueError(f"checkpoint was trained with sampled_loss={saved_loss!r}, the model has sampled_loss={my_loss!r}: a resumed "
                         "run keeps its objective")
    with torch.no_grad():
        model._arena.copy_(ck["arena"])
        model._adam_m.copy_(ck["adam_m"])
        model._adam_v.copy_(ck["adam_v"])
        model._adam_state.copy_(ck["adam_state"])
        model._rng_state.copy_(ck["rng_state"])
    model.neg_step = int(ck.get("neg_step", 0))      # (optional field: sampled training steps taken)
    if getattr(model, "lazy_adam", False):           # (the claim words are not saved; the step count may have gone back)
        model._stamp.zero_()
        model.zero_grad_arena()
    model._state_ahead = False     # the file holds "steps taken" (save_checkpoint settles the engine's look-ahead)
    model.sync_shadow()


def regressive_batch(tok, tim, is_training: bool):
    """RegressivePostProcessor (dataloader.py:88-108; util.reader's choice for CTSMA / TGAT / TiSASREC, util.py:116-129):
    features see tokens[:-1] and every timestamp; labels = tokens[1:] (training) / the whole record (evaluation)."""
    return {"seqs_i": tok[:, :-1].contiguous(), "seqs_t": tim}, (tok[:, 1:].contiguous() if is_training else tok)


def regressive_calendar_batch(tok, tim, cal, is_training: bool):
    """regressive_batch with RegressivePostProcessor(has_datetime=True)'s four calendar fields (dataloader.py:95-108; TimelyREC):
    `cal` = (month, day, weekday, hour) int64 [B, T+1]; the features see field[:-1]."""
    feats, labels = regressive_batch(tok, tim, is_training)
    for name, a in zip(("seqs_month", "seqs_day", "seqs_weekday", "seqs_hour"), cal):
        feats[name] = a[:, :-1].contiguous()
    return feats, labels


def load_calendar_or_derive(patterns, seqslen, ids, ts, split):
    """The split's calendar fields from its files, or — files without them — derived from the timestamps (UTC), with one log line."""
    from . import formats as F
    try:
        return F.load_calendar(patterns, seqslen)
    except KeyError:
        logging.info("   %s: no calendar fields in the files; derived from seqs_t (UTC)", split)
        return F.calendar_from_timestamps(ts, ids)


def evaluate(model, ids, ts, batch_size: int, mask_seen: bool, loader=None, by_rank: bool = False, negatives: int = 0,
             neg_seed: int = 0, neg_dist=None, calendar=None) -> Dict[str, float]:
    """One pass of ``Sequential.eval`` (Base.py:150-207) over a split: last position masked (EasyDGL) or predicted from the
    prefix (regressive models), streaming means.  `loader`: a data.DeviceLoader in an evaluation mode over the resident split
    (--device_data) — the batches are then assembled on the device, in file order.  `by_rank`: the metrics from the label's rank
    (model.eval_step(by_rank=True)) — the same H / N values plus "MRR".  `negatives` > 0: the sampled-negative protocol —
    the label ranked among that many negatives per sequence, keyed by (neg_seed, step 0, the sequence's index in the split): every
    pass over a split ranks against the same lists, whatever the batch size; cut-offs (1, 5, 10).  `neg_dist` (ops.NegDist): those
    negatives are drawn by its weights.  `calendar`: the split's four calendar arrays (TimelyREC)."""
    import torch
    from . import data as D
    if negatives > 0:
        model.reset_metrics((1, 5, 10))
        row0 = [0]      # running sequence offset of the split
        extra = {} if neg_dist is None else {"neg_dist": neg_dist}

        def step(feats, labels):
            model.eval_step(feats, labels, mask_seen=mask_seen, negatives=negatives, neg_seed=neg_seed, row0=row0[0], **extra)
            row0[0] += labels.shape[0]
    else:
        model.reset_metrics()

        def step(feats, labels):
            model.eval_step(feats, labels, mask_seen=mask_seen, by_rank=by_rank)
    if loader is not None:
        loader.set_epoch(None)
        for _ in range(len(loader)):
            feats, labels = loader.next()
            step(feats, labels)
        return model.metrics()
    n = ids.shape[0]
    masked = hasattr(model, "mask")
    for lo in range(0, n, batch_size):
        tok = torch.as_tensor(ids[lo:lo + batch_size]).cuda()
        tim = torch.as_tensor(ts[lo:lo + batch_size]).cuda()
        if calendar is not None:
            cal = [torch.as_tensor(a[lo:lo + batch_size]).cuda() for a in calendar]
            feats, labels = regressive_calendar_batch(tok, tim, cal, False)
        else:
            feats, labels = D.device_mask_last(tok, tim, model.mask) if masked else regressive_batch(tok, tim, False)
        step(feats, labels)
    return model.metrics()


def run(FLAGS) -> Dict[str, float]:
    import torch
    from . import data as D
    from . import formats as F
    from .engine import TrainEngine
    from .util import ranking

    torch.manual_seed(FLAGS.seed)
    rng = np.random.default_rng(FLAGS.seed)
    logging.info("1. read data")
    tr_i, tr_t = F.load_sequences(FLAGS.train, FLAGS.seqslen)
    vl_i, vl_t = F.load_sequences(FLAGS.valid, FLAGS.seqslen)
    te_i, te_t = F.load_sequences(FLAGS.test, FLAGS.seqslen)
    logging.info("   train %d, valid %d, test %d sequences of %d positions", len(tr_i), len(vl_i), len(te_i), tr_i.shape[1])

    cals = None
    if FLAGS.model == "TimelyREC":
        # the on-device loader and graph capture know nothing of the calendar fields (out of scope)
        if getattr(FLAGS, "device_data", False):
            raise ValueError("--device_data with --model TimelyREC: the on-device loader does not carry the calendar fields")
        if getattr(FLAGS, "graph", False):
            raise ValueError("--graph with --model TimelyREC: its step is not captured into a graph; run without --graph")
        cals = {"train": load_calendar_or_derive(FLAGS.train, FLAGS.seqslen, tr_i, tr_t, "train"),
                "valid": load_calendar_or_derive(FLAGS.valid, FLAGS.seqslen, vl_i, vl_t, "valid"),
                "test": load_calendar_or_derive(FLAGS.test, FLAGS.seqslen, te_i, te_t, "test")}

    logging.info("2. create neural model")
    if getattr(FLAGS, "mark", None) and isinstance(FLAGS.mark, str):
        FLAGS.mark_table = F.load_mark_table(FLAGS.mark, FLAGS.num_items)
    FLAGS.compute_dtype = getattr(FLAGS, "dtype", "bf16")
    if getattr(FLAGS, "deterministic", False) and FLAGS.model != "EasyDGL":
        # The regressive models have their ordered forms too and take the mode through FLAGS.deterministic /
        # ranking(FLAGS); this driver keeps its refusal for them (tests/test_cpu_segsum.py pins it: lifting it is a change of
        # existing behaviour of its own).  The promise must never silently not hold.
        raise ValueError(f"--deterministic: this driver runs the mode for --model EasyDGL only (got {FLAGS.model}); "
                         f"build the model with FLAGS.deterministic instead: DESIGN 4.9")
    model = ranking(FLAGS)
    model.finalize(torch.device("cuda", torch.cuda.current_device()))
    bs = FLAGS.batch_size
    masked = FLAGS.model == "EasyDGL"          # MAUPostProcessor; every other model is fed regressively (util.py:99-129)
    if FLAGS.model == "TGAT":                  # the time feature map needs time-sorted sequences (model/tgat.py)
        for name, (ii, tt) in (("train", (tr_i, tr_t)), ("valid", (vl_i, vl_t)), ("test", (te_i, te_t))):
            if np.any((np.diff(tt, axis=1) < 0) & (ii[:, :-1] != 0)):
                raise ValueError(f"{name}: timestamps decrease inside a sequence; TGAT needs time-sorted records")
    device_data = bool(getattr(FLAGS, "device_data", False))
    by_rank = bool(getattr(FLAGS, "eval_by_rank", False))     # (the default cut-offs keep "H100": early stopping reads it either way)
    negatives, neg_seed = int(getattr(FLAGS, "eval_negatives", 0) or 0), int(getattr(FLAGS, "eval_neg_seed", 0) or 0)
    select_on = "H10" if negatives > 0 else "H100"            # (H100 of N + 1 <= 101 candidates is constant)
    # --device_data --graph: the batch no longer arrives from the host, so the EasyDGL step can be replayed as one graph
    engine_graph = device_data and bool(getattr(FLAGS, "graph", False))
    train_negatives = int(getattr(FLAGS, "train_negatives", 0) or 0)
    if train_negatives > 0 and getattr(FLAGS, "graph", False):
        raise ValueError("--graph with --train_negatives: the sampled-softmax step runs on the autograd path (model.train_step)")
    shared_negatives = int(getattr(FLAGS, "shared_negatives", 0) or 0)
    if shared_negatives > 0 and getattr(FLAGS, "graph", False):
        raise ValueError("--graph with --shared_negatives: the sampled-softmax step runs on the autograd path (model.train_step)")
    # weighted negatives: the counts are one bincount of the training split's item ids (the host copy, with
    # --device_data too), so a resumed run rebuilds the same table
    neg_sampler = str(getattr(FLAGS, "neg_sampler", None) or "uniform")
    eval_dist = None
    if neg_sampler == "popularity" or getattr(FLAGS, "eval_neg_sampler", "uniform") == "popularity":
        from . import ops
        hi = model._negatives_hi()
        counts = np.bincount(np.asarray(tr_i).reshape(-1).astype(np.int64), minlength=hi)
        w = ops.neg_weights("popularity", hi, 1, hi, counts, float(getattr(FLAGS, "neg_alpha", 0.75)))
        if neg_sampler == "popularity":
            model.set_negative_weights(w)
        if getattr(FLAGS, "eval_neg_sampler", "uniform") == "popularity":
            eval_dist = model.negative_dist(w, T_reject=int(vl_i.shape[1]))       # (a sequence rejects its history and its label)
    # sampled-softmax training: no static engine, every batch through model.train_step
    engine =TrainEngine(model, bs, use_graph=engine_graph) if (masked and len(tr_i) >= bs and train_negatives <= 0 and shared_negatives <= 0) else None
    loader = vl_loader = te_loader = None
    if device_data:
        need = sum(D.DeviceSplit.nbytes(ii, tt) + 4 * len(ii) for ii, tt in ((tr_i, tr_t), (vl_i, vl_t), (te_i, te_t)))
        free = torch.cuda.mem_get_info()[0]
        if need > free:
            raise RuntimeError(f"--device_data: the splits need {need} bytes of device memory, {free} bytes are free; "
                               "run without --device_data (batches from the host)")
        mask_id = int(model.mask) if masked else 0
        loader = D.DeviceLoader(D.DeviceSplit(tr_i, tr_t), bs, "mask_random" if masked else "regressive_train", mask_id,
                                FLAGS.masklen if masked else 0, FLAGS.seed)
        emode = "mask_last" if masked else "regressive_eval"
        vl_loader = D.DeviceLoader(D.DeviceSplit(vl_i, vl_t), bs, emode, mask_id)
        te_loader = D.DeviceLoader(D.DeviceSplit(te_i, te_t), bs, emode, mask_id)
        logging.info("   splits resident on the device: %d bytes", need)
        if engine is not None:
            engine.attach_loader(loader)
    if engine is not None:
        # the loss is read every 10 batches (NaN test) and once per epoch: the engine leaves its loss launches off the step
        # (they ride with the next step) and adds the step losses up on the device — the mode bench.py times
        engine.sync_loss = False
        engine.accumulate_loss = True
    ckpt = os.path.join(FLAGS.ckpt_dir, f"{FLAGS.model}.pt")
    stopper = EarlyStopping(FLAGS.model, patience=FLAGS.patience, saver=lambda: save_checkpoint(model, ckpt))
    mask_state = torch.tensor([FLAGS.seed, 0], dtype=torch.int64, device="cuda")   # (seed, batch counter) of the masker
    gstep = None

    logging.info("3. train and evaluate model")
    for epoch in range(FLAGS.num_epochs):
        order = rng.permutation(len(tr_i))
        # streaming epoch mean of the step losses, as tf.metrics.mean feeds EarlyStopping in the reference (Base.py:133-134,
        # main.py:119-122); accumulated on the device, read back every 10 batches for the NaN test and once per epoch
        loss_sum = torch.zeros((), device="cuda", dtype=torch.float64)
        running_loss, nb = float("nan"), 0
        if engine is not None:
            engine.join_loss()
            engine.loss_sum.zero_()
        if loader is not None:
            loader.set_epoch(order)      # the one upload of the epoch: same order, hence the same batches and mask draws as below
        for lo in range(0, len(order), bs):
            idx = order[lo:lo + bs]
            if loader is not None:
                # full EasyDGL batches: the attached loader writes the engine's buffers inside engine.step(); everything else
                # (remainder batch, regressive models) takes fresh tensors from the same device cursor
                feats, labels = (None, None) if (engine is not None and len(idx) == bs) else loader.next()
            else:
                tok = torch.as_tensor(tr_i[idx]).cuda()
                tim = torch.as_tensor(tr_t[idx]).cuda()
                if masked:
                    feats, labels = D.device_mask_random(tok, tim, model.mask, FLAGS.masklen, mask_state)
                    mask_state[1] += 1
                elif cals is not None:
                    feats, labels = regressive_calendar_batch(tok, tim, [torch.as_tensor(a[idx]).cuda() for a in cals["train"]], True)
                else:
                    feats, labels = regressive_batch(tok, tim, True)
            if engine is not None and len(idx) == bs:
                engine.step(feats, labels)
                loss = None      # (added to engine.loss_sum by the engine's own loss launches)
            elif not masked and getattr(FLAGS, "graph", False) and len(idx) == bs:
                if gstep is None:
                    # the warm-up step that precedes the capture IS this batch's optimizer step: no replay for it
                    gstep = model.graphed_train_step(feats, labels, warmup=1)
                    loss = gstep.warmup_loss
                else:
                    loss = gstep(feats, labels)
            else:
                loss = model.train_step(feats, labels)
            nb += 1
            if loss is not None:
                loss_sum += loss.reshape(()).double()
            if nb % 10 == 0 or lo + bs >= len(order):
                if engine is not None:
                    engine.join_loss()       # orders this stream behind the (deferred) loss launches of the last step
                running_loss = (float(loss_sum) + (float(engine.loss_sum) if engine is not None else 0.0)) / nb
                if math.isnan(running_loss):
                    break
        logging.info("%03d: Loss=%.4f", epoch, running_loss)
        if hasattr(model, "check_inputs"):
            model.check_inputs()
        if math.isnan(running_loss):      # util.py:29-30: a NaN loss stops the run, whatever eval_per_steps says
            stopper.step(running_loss, 0.0, {}, {})
            break
        if epoch % FLAGS.eval_per_steps:
            continue
        vl = evaluate(model, vl_i, vl_t, bs, FLAGS.mask_seen, vl_loader, by_rank, negatives, neg_seed, eval_dist,
                      None if cals is None else cals["valid"])
        logging.info("%03d: %s", epoch, {k: "{0:.5f}".format(v) for k, v in vl.items()})
        te = evaluate(model, te_i, te_t, bs, FLAGS.mask_seen, te_loader, by_rank, negatives, neg_seed, eval_dist,
                      None if cals is None else cals["test"])
        if stopper.step(running_loss, vl[select_on], vl, te):
            break
    return stopper.summary()


def main(argv=None):
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(message)s")
    FLAGS = args(argv)
    return run(SimpleNamespace(**vars(FLAGS)))


if __name__ == "__main__":
    main()
