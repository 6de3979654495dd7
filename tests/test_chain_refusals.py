"""The eight entry points of the fused latent chains refuse bad arguments before any launch, each with its message, and their no-ops
look at no pointer (tests/chain_refusals.py): no device needed.  The fp32 and the bf16 entries share their operand checks
(csrc/gauss_chain_common.h); this table pins what a caller reads, per entry and per head."""
import pytest

import chain_refusals as CR


@pytest.mark.parametrize("name", sorted(CR.ENTRIES))
def test_entry_refuses_and_no_ops_without_a_device(name):
    from s2p_amd import _lib
    e = CR.ENTRIES[name]
    n = CR.check(_lib, name)
    # sizes, the entry's own operands, and seven cases per head
    assert n >= 2 + 7 * len(e.heads) + (15 if e.bwd else 13)


def test_tables_name_the_mode_and_the_heads():
    """The row multiple is worded per mode, every head of an entry is named, and every edit differs."""
    for name, e in CR.ENTRIES.items():
        table = CR.cases(name)
        texts = [t for _, t in table]
        assert len({repr(sorted(c.items())) + t for c, t in table}) == len(table), name
        unit, other = ("8 bf16 elements", "4 floats and at least K") if e.bf16 else ("4 floats", "8 bf16 elements")
        assert any(unit in t for t in texts) and not any(other in t for t in texts), name
        for head, k in e.heads:
            assert sum(t.startswith(head + ":") for t in texts) >= 7, (name, head)
    assert set(CR.ENTRIES) == {"s2p_posterior_chain_fwd", "s2p_posterior_chain_fwd_save", "s2p_posterior_chain_bwd", "s2p_prior_chain_fwd",
                               "s2p_imagine_chain_fwd", "s2p_posterior_chain_fwd_bf16", "s2p_prior_chain_fwd_bf16",
                               "s2p_imagine_chain_fwd_bf16"}
