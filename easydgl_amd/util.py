"""Mirror of src/util.py:ranking — the model factory that is the reference's only plugin API."""


def ranking(FLAGS):
    """util.py:61-96.  Only the models on the accelerated path exist here."""
    if FLAGS.model == "EasyDGL":
        from .model import EasyDGL
        return EasyDGL(FLAGS.num_items, FLAGS)
    if FLAGS.model == "TGAT":
        from .model import TGAT
        return TGAT(FLAGS.num_items, FLAGS)
    if FLAGS.model == "TiSASREC":
        from .model import TiSASRec
        return TiSASRec(FLAGS.num_items, FLAGS)
    if FLAGS.model == "CTSMA":
        from .model import CTSMA
        return CTSMA(FLAGS.num_items, FLAGS)
    if FLAGS.model == "SASREC":
        from .model import SASRec
        return SASRec(FLAGS.num_items, FLAGS)
    if FLAGS.model == "S2PNM":
        from .model import S2PNM
        return S2PNM(FLAGS.num_items, FLAGS)
    if FLAGS.model == "TimelyREC":
        from .model import TimelyREC
        return TimelyREC(FLAGS.num_items, FLAGS)
    if FLAGS.model == "TGREC":
        from .model import TGREC
        return TGREC(FLAGS.num_items, FLAGS)
    # GREC is built from a flags object that carries the model's flags (the driver's and every caller's that sets num_items); a
    # namespace with nothing but the model name keeps the answer it had before the model existed (tests/test_cpu_seq_baselines.py
    # pins it), i.e. it falls through to the refusal below
    if FLAGS.model == "GREC" and hasattr(FLAGS, "num_items"):
        from .model import GREC
        return GREC(FLAGS.num_items, FLAGS)
    if FLAGS.model == "BERT4REC" and hasattr(FLAGS, "num_items"):     # (as GREC: the bare namespace keeps its refusal)
        from .model import BERT4REC
        return BERT4REC(FLAGS.num_items, FLAGS)
    if FLAGS.model == "GRU4REC" and hasattr(FLAGS, "num_items"):      # (as GREC: the bare namespace keeps its refusal)
        from .model import GRU4REC
        return GRU4REC(FLAGS.num_items, FLAGS)
    if FLAGS.model == "NARM" and hasattr(FLAGS, "num_items"):         # (not a reference model; guarded like its neighbours)
        from .model import NARM
        return NARM(FLAGS.num_items, FLAGS)
    raise NotImplementedError("The ranking model: {0} not implemented".format(FLAGS.model))
