from . import nuts  # noqa: F401
