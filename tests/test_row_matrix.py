"""CPU test of tests/row_matrix.py: the grid of (MAXIT, BCRT, MASS) kernel instances against the case tables of the GPU tests.  The five
families GHMC, MEADS, ChEES, ``mfm_hmc_run_lengths`` and HMC with an installed mass reach every cell; for every other entry point the
unreached cells are exactly the ``OPEN`` set written out in the helper."""
import pytest

from tests import row_matrix as rm


def _show(cells):
    return sorted(cells, key=str)


def test_the_derivation_follows_the_dispatch():
    assert [rm.cell(d, False)[0] for d in (2, 64, 65, 256, 257, 1024, 1025, 2048)] == [1, 1, 4, 4, 16, 16, 32, 32]
    assert rm.cell(289, True, True) == (16, True, True)
    assert len(rm.grid("mala_step")) == 8 and len(rm.grid("meads_step")) == 8 and len(rm.grid("ghmc_step")) == 16
    assert all(ms for _, _, ms in rm.grid("meads_step"))
    # every entry point that goes through ROW_DISPATCH / HMC_MASS_DISPATCH is listed
    assert set(rm.ENTRY_POINTS) == {"mala_init", "loglik", "mala_step", "hmc_step", "mala_run", "hmc_run", "mala_warmup", "hmc_warmup",
                                    "hmc_warmup_window", "mclmc_step", "mclmc_run", "ghmc_step", "ghmc_run", "meads_step", "chees_step",
                                    "hmc_run_lengths", "pt_hmc_run", "pt_mala_run", "pt_exchange"}
    for entry in rm.ENTRY_POINTS:
        assert rm.reached(entry) <= rm.grid(entry), (entry, _show(rm.reached(entry) - rm.grid(entry)))     # no mass case on a kernel without MASS


@pytest.mark.parametrize("family", rm.FAMILIES)
def test_the_five_families_reach_every_cell(family):
    """For phi-four every (MAXIT, BCRT) cell, with and without a mass where the kernel has MASS instances (MEADS: always with)."""
    print(family, "reaches", _show(rm.reached(family)))
    assert not rm.unreached(family), (family, _show(rm.unreached(family)))
    assert family not in rm.OPEN
    if family != "hmc_mass":
        assert rm.reaches_the_mixture(family), family               # and the mixture path, which exists at MAXIT 1, BCRT false only


@pytest.mark.parametrize("entry", [e for e in rm.ENTRY_POINTS if e not in rm.FAMILIES])
def test_the_open_set_is_exactly_the_unreached_cells(entry):
    """It can shrink (strike the cell from ``OPEN`` with the case that closes it); it cannot grow unnoticed."""
    assert entry in rm.OPEN, entry
    print(entry, "open", {c: why for c, why in rm.OPEN[entry].items()})
    assert set(rm.OPEN[entry]) == rm.unreached(entry), (entry, _show(set(rm.OPEN[entry]) ^ rm.unreached(entry)))
    assert all(isinstance(why, str) and why for why in rm.OPEN[entry].values())
