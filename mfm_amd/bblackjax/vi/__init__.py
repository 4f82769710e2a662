from . import svgd  # noqa: F401  (the module, as bblackjax.vi.svgd: its class of the same name is svgd.svgd)
