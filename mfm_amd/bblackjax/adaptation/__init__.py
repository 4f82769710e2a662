"""Adaptation drivers, where the reference's ``bblackjax`` keeps its own (``bblackjax/adaptation``): ``window_adaptation``, ``chees_adaptation``, ``meads_adaptation``."""
