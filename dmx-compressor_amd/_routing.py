"""The `fused=None | True | False` protocol every kernel family of `_front.py` follows, written once, with what goes with it: the
straight-through tail of the dynamic casts and the piece loop of their chains.

No module state and no raw namespace: `ops.front(binding)` executes `_front.py` a second time over the other binding, both copies
import this module, and each passes in its own counters.
"""
import torch

DYNAMIC_CHAIN_MAX_SEGMENTS = 65535   # groups of one dmxq_group_minmax call; more segments: the chain runs on pieces of ...
DYNAMIC_CHAIN_PIECE = 32768          # ... this many segments (the kernel has no such limit)


def route(fused, key, chain_by_default, routes, kernel, chain, refuse):
    """One front-end call's choice between its kernel and its chain -> what the chosen one returns.
    key: None where the kernel does not apply, else what the family's *_CHAIN_BY_DEFAULT set lists (a geometry class name; the group
    size M in Wanda and AWQ, where 0 is a key like any other).  The caller forms it only where `fused is not False`: that asks the
    library, and fused=False must not.  kernel / chain: zero-argument callables.  refuse: a zero-argument callable that returns the
    NotImplementedError's text, called only where it is raised.  routes: the family's {"fused", "chain"} counters, or None.
    fused=False: the chain.  No key: NotImplementedError under fused=True, else the chain.  fused=None and the key listed: the chain.
    Otherwise the kernel, counted once it has returned; its NotImplementedError (DMXQ_ERR_UNSUPPORTED, nothing launched) is raised again
    under fused=True and sends the call to the chain otherwise.  The chain is counted before it runs."""
    if fused is not False:
        if key is None:
            if fused:
                raise NotImplementedError(refuse())
        elif fused is not None or key not in chain_by_default:
            try:
                out = kernel()
                if routes is not None:
                    routes["fused"] += 1
                return out
            except NotImplementedError:
                if fused:
                    raise
    if routes is not None:
        routes["chain"] += 1
    return chain()


class _DynamicSTE(torch.autograd.Function):
    """the dynamic cast as a straight-through estimator (cast.py _FixedAffineCast: the scales are not differentiated either)"""

    @staticmethod
    def forward(ctx, x, run):
        ctx.set_materialize_grads(False)
        ctx.in_dtype = x.dtype
        out = run(x.detach())
        if isinstance(out, tuple):
            ctx.mark_non_differentiable(*out[1:])
        return out

    @staticmethod
    def backward(ctx, g, *_):
        if g is not None and g.dtype != ctx.in_dtype:
            g = g.to(ctx.in_dtype)
        return g, None


def straight_through(x, run):
    """run(x.detach()): under autograd as a straight-through estimator (_DynamicSTE), else without a graph"""
    if not torch.is_grad_enabled():
        return run(x.detach())
    if x.requires_grad:
        return _DynamicSTE.apply(x, run)
    # torch.no_grad() by its two function calls: entering the context manager costs more host time than route() and its closures do
    torch.set_grad_enabled(False)
    try:
        return run(x.detach())
    finally:
        torch.set_grad_enabled(True)


def in_pieces(chain, x2, n_out):
    """chain(x2) -> a tuple of n_out per-segment outputs (tensors; None for one that was not asked for) over the rows of x2 [n, S].
    dmxq_group_minmax takes 65535 groups: segments are independent, so above DYNAMIC_CHAIN_MAX_SEGMENTS rows the chain runs on pieces of
    DYNAMIC_CHAIN_PIECE rows and the results are joined."""
    if x2.shape[0] <= DYNAMIC_CHAIN_MAX_SEGMENTS:
        return chain(x2)
    parts = [chain(x2[i:i + DYNAMIC_CHAIN_PIECE]) for i in range(0, x2.shape[0], DYNAMIC_CHAIN_PIECE)]
    return tuple(None if parts[0][k] is None else torch.cat([p[k] for p in parts]) for k in range(n_out))
