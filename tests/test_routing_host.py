"""-m "not gpu": the fused=None | True | False protocol of the front ends (dmx-compressor_amd/_routing.py) as a truth table over fake
kernel / chain callables -- which one ran, what was raised, the exact counter deltas, the lazy refusal text -- and the piece loop of
the chains on a CPU tensor."""
import itertools

import pytest
import torch

from dmx_compressor_amd import _routing as R

LISTED = frozenset({"a", 0})


def expected(fused, key, listed, refuses):
    """the protocol, spelled as a table: -> (what the call gives, the order the callables ran in)"""
    if fused is False:
        return "chain", ["chain"]
    if key is None:
        return ("refused", ["refuse"]) if fused else ("chain", ["chain"])
    if fused is None and listed:
        return "chain", ["chain"]
    if not refuses:
        return "kernel", ["kernel"]
    return ("unsupported", ["kernel"]) if fused else ("chain", ["kernel", "chain"])


@pytest.mark.parametrize("fused, key, listed, refuses", list(itertools.product([None, True, False], [None, "a", 0], [True, False], [False, True])))
def test_route_truth_table(fused, key, listed, refuses):
    ran = []
    routes = {"fused": 0, "chain": 0}
    at_chain = []

    def kernel():
        ran.append("kernel")
        assert routes == {"fused": 0, "chain": 0}   # nothing is counted before the kernel has returned
        if refuses:
            raise NotImplementedError("DMXQ_ERR_UNSUPPORTED")
        return "kernel"

    def chain():
        ran.append("chain")
        at_chain.append(dict(routes))
        return "chain"

    def refuse():
        ran.append("refuse")
        return "no kernel for this call"

    want, order = expected(fused, key, listed, refuses)
    args = (fused, key, LISTED if listed else frozenset(), routes, kernel, chain, refuse)
    if want in ("refused", "unsupported"):
        with pytest.raises(NotImplementedError) as e:
            R.route(*args)
        assert str(e.value) == ("no kernel for this call" if want == "refused" else "DMXQ_ERR_UNSUPPORTED")
        assert routes == {"fused": 0, "chain": 0}
    else:
        assert R.route(*args) == want
        assert routes == {"fused": int(want == "kernel"), "chain": int(want == "chain")}
    assert ran == order   # (the refusal text is formed only where it is raised)
    assert at_chain == ([{"fused": 0, "chain": 1}] if want == "chain" else [])   # the chain is counted before it runs


def test_route_without_counters_and_other_errors():
    def broken():
        raise ValueError("an argument error of the kernel's own")

    assert R.route(None, "a", frozenset(), None, lambda: "kernel", lambda: "chain", None) == "kernel"
    assert R.route(False, "a", frozenset(), None, None, lambda: "chain", None) == "chain"
    routes = {"fused": 0, "chain": 0}
    with pytest.raises(ValueError):
        R.route(None, "a", frozenset(), routes, broken, lambda: "chain", None)
    assert routes == {"fused": 0, "chain": 0}


def test_in_pieces_joins_the_pieces_and_keeps_none():
    n = R.DYNAMIC_CHAIN_MAX_SEGMENTS + 1
    x2 = torch.arange(2 * n, dtype=torch.float32).reshape(n, 2)
    sizes = []

    def chain(part):
        sizes.append(part.shape[0])
        return part * 2.0, part.sum(dim=1), None

    y, s, nothing = R.in_pieces(chain, x2, 3)
    assert sizes == [R.DYNAMIC_CHAIN_PIECE] * 2 and sum(sizes) == n
    assert torch.equal(y, x2 * 2.0) and torch.equal(s, x2.sum(dim=1)) and nothing is None
    del sizes[:]
    y, s, nothing = R.in_pieces(chain, x2[:-1], 3)   # what one group_minmax call takes: one piece
    assert sizes == [n - 1] and torch.equal(y, x2[:-1] * 2.0) and torch.equal(s, x2[:-1].sum(dim=1)) and nothing is None


def test_straight_through_passes_the_gradient_and_detaches_without_one():
    def run(xd):
        assert not xd.requires_grad
        return (xd * 0.0).to(torch.float64), xd.new_ones(1)

    x = torch.ones(3, requires_grad=True)
    y, s = R.straight_through(x, run)
    assert y.requires_grad and not s.requires_grad
    y.sum().backward()
    assert x.grad.dtype == torch.float32 and torch.equal(x.grad, torch.ones(3))   # the identity, in the input's dtype
    with torch.no_grad():
        assert not R.straight_through(x, run)[0].requires_grad
    assert not R.straight_through(x.detach(), run)[0].requires_grad

    def broken(xd):
        assert not torch.is_grad_enabled()
        raise ValueError("from the cast")

    with pytest.raises(ValueError):
        R.straight_through(x.detach(), broken)
    assert torch.is_grad_enabled()   # the grad mode comes back after an error too


def test_the_front_end_keeps_the_piece_constants_under_its_own_names(dmx):
    F = dmx.ops._front
    assert (F.DYNAMIC_CHAIN_MAX_SEGMENTS, F.DYNAMIC_CHAIN_PIECE) == (R.DYNAMIC_CHAIN_MAX_SEGMENTS, R.DYNAMIC_CHAIN_PIECE) == (65535, 32768)
