from . import feeder_nucla_gcn   # noqa: F401
from . import clip_feeder        # noqa: F401
