"""The scratch sizes of the four batch ops that carve their arrays out of the
caller's scratch (pptk_amd/csrc/scratch_carve.h), pinned to literals.  The
numbers are what the library returned before the ops' layouts moved onto the
shared carver (the three-list layouts of ip_reass.hip, rx_flowlearn.hip,
tx_dispatch.hip and tx_frag.hip): a caller's allocation of that size stays
large enough, and the arrays stay where they were."""
import pytest

from pptk_amd.rx import (flow_learn_scratch_bytes, ip_reass_scratch_bytes, lib,
                         tx_dispatch_scratch_bytes)

LEARN = {(1, 1): 1280, (1000, 10): 1792, (1000, 1000): 41728, (4097, 4096): 164608,
         (10**6, 1000): 42496, (2**32 - 1, 2**30): 42970644992}
REASS = {(1, 1): 3584, (1000, 10): 4352, (1000, 1000): 115456, (2**24, 2**24): 1879834880}
DISPATCH = {(1, 1): 512, (4096, 4): 512, (4097, 64): 4608, (10**7, 64): 2561536,
            (2**32 - 1, 64): 1098909952}
FRAGMENT = {0: 64, 1: 144, 255: 4432, 256: 4432, 257: 4496, 2**24: 285737024}


@pytest.mark.parametrize("args", sorted(LEARN))
def test_flow_learn_scratch_bytes(args):
    assert flow_learn_scratch_bytes(*args) == LEARN[args]


@pytest.mark.parametrize("args", sorted(REASS))
def test_ip_reass_scratch_bytes(args):
    assert ip_reass_scratch_bytes(*args) == REASS[args]


@pytest.mark.parametrize("args", sorted(DISPATCH))
def test_tx_dispatch_scratch_bytes(args):
    assert tx_dispatch_scratch_bytes(*args) == DISPATCH[args]


@pytest.mark.parametrize("n", sorted(FRAGMENT))
def test_ip_fragment_scratch_bytes(n):
    assert lib().pptk_ip_fragment_scratch_bytes(n) == FRAGMENT[n]
