from . import nuts  # noqa: F401
from . import elliptical_slice  # noqa: F401
from . import mclmc  # noqa: F401
from . import ghmc  # noqa: F401
