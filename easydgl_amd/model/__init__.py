from .base import Sequential  # noqa: F401
from .easydgl import EasyDGL  # noqa: F401
from .ctsma import CTSMA  # noqa: F401
from .tgat import TGAT  # noqa: F401
from .tisasrec import TiSASRec  # noqa: F401
from .sasrec import SASRec  # noqa: F401
from .s2pnm import S2PNM  # noqa: F401
from .timelyrec import TimelyREC  # noqa: F401
