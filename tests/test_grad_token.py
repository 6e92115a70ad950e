"""hip_conv.GradToken: the gradient hand-off between a producer P, the finisher of its output's gradient and the other
consumers (depositors) is host logic.  Driven here with small CPU tensors, torch adds standing in for the launches."""
import pytest
import torch

from oadg_amd import hip_conv, hip_ops
from oadg_amd.hip_conv import GradToken


def _g(seed, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(1, 8, 2, 3, generator=g).to(dtype).contiguous(memory_format=torch.channels_last)


def _conv_deposit(tok, g):
    """what _Conv2dMFMA.backward does with a ``dep_token`` and the data gradient ``g``: None when it was deposited"""
    if not tok.may_deposit():
        return g
    extra = tok.take()
    tok.leave(g if extra is None else g + extra)
    return None


def _finish(tok, g):
    """the finisher's backward: close, add what was deposited in the "launch", leave the column sums"""
    extra = tok.close()
    gx = g if extra is None else g + extra
    return tok.finish(gx, gx.float().sum((0, 2, 3)))


def test_depositors_then_finisher_then_producer():
    tok = GradToken()
    assert not tok.adopted and not tok.armed and not tok.closed
    tok.arm()
    g1, g2, g3 = _g(1), _g(2), _g(3)
    assert _conv_deposit(tok, g1) is None and hip_ops._deposit((tok,), (g2,)) == [None]
    assert torch.equal(tok.extra, g1 + g2)
    gx = _finish(tok, g3)
    assert tok.closed and tok.extra is None and tok.grad_ptr == gx.data_ptr()
    assert torch.equal(gx, g3 + (g1 + g2))
    colsum = tok.colsum
    trusted, cs = tok.claim(gx)
    assert trusted and cs is colsum and torch.equal(cs, gx.float().sum((0, 2, 3)))
    assert tok.grad_ptr is None and tok.colsum is None
    assert tok.claim(gx) == (False, None)                # the hand-off is spent


@pytest.mark.parametrize('form', ['conv', 'tensor'])
def test_late_depositor_gets_its_gradient_back_and_taints(form):
    tok = GradToken()
    tok.arm()
    gx = _finish(tok, _g(1))
    g = _g(2)
    back = _conv_deposit(tok, g) if form == 'conv' else hip_ops._deposit([tok], [g])[0]
    assert back is g and tok.extra is None
    assert tok.grad_ptr is None and tok.colsum is None
    assert tok.claim(gx) == (False, None)                # even with the matching pointer


def test_never_armed_token_takes_nothing():
    tok = GradToken()
    g, gx = _g(1), _g(2)
    tok.finish(gx, gx.float().sum((0, 2, 3)))            # (a pointer a taint would clear)
    assert _conv_deposit(tok, g) is g and hip_ops._deposit([tok], [g]) == [g]
    assert tok.extra is None and not tok.closed
    assert tok.grad_ptr == gx.data_ptr() and tok.colsum is not None


@pytest.mark.parametrize('case', ['other_tensor', 'fp32', 'not_channels_last'])
def test_untrusted_claims_clear_the_token(case):
    tok = GradToken()
    tok.arm()
    gx = _finish(tok, _g(1))
    if case == 'other_tensor':
        gy = gx.clone()
    elif case == 'fp32':
        gy = gx.float()
        tok.finish(gy, tok.colsum)                       # (the pointer matches: the dtype alone must refuse it)
    else:
        gy = _g(1).contiguous()                          # bf16, NCHW-contiguous
        assert not gy.is_contiguous(memory_format=torch.channels_last)
        tok.finish(gy, tok.colsum)
    assert tok.grad_ptr is not None
    assert tok.claim(gy) == (False, None)
    assert tok.grad_ptr is None and tok.colsum is None


def test_tensor_deposit_takes_bf16_only():
    tok = GradToken(masked=False)
    tok.arm()
    g32, gx = _g(1, torch.float32), _g(4)
    tok.finish(gx, gx.float().sum((0, 2, 3)))            # (a pointer a taint would clear)
    assert hip_ops._deposit([tok, None], [g32, g32]) == [g32, g32]
    assert tok.extra is None and not tok.closed
    assert tok.grad_ptr == gx.data_ptr() and tok.colsum is not None
    g1, g2 = _g(2), _g(3)
    assert hip_ops._deposit([tok], [g1]) == [None] and tok.extra is g1
    assert hip_ops._deposit([tok], [g2]) == [None] and torch.equal(tok.extra, g1 + g2)
    assert hip_ops._deposit(None, [g1]) == [g1]


def test_deposit_switch_off_still_taints(monkeypatch):
    monkeypatch.setattr(hip_conv, 'DEPOSIT', False)
    tok = GradToken()
    tok.arm()
    g = _g(1)
    assert _conv_deposit(tok, g) is g and hip_ops._deposit([tok], [g]) == [g]
    assert tok.extra is None
    gx = _finish(tok, _g(2))
    assert tok.grad_ptr == gx.data_ptr()
    assert _conv_deposit(tok, g) is g                    # closed: tainted, whatever the switch says
    assert tok.grad_ptr is None and tok.colsum is None


@pytest.mark.parametrize('armed', [True, False])
def test_identity_hand_off_is_unconditional(armed):
    tok = GradToken()
    if armed:
        tok.arm()
    gy = _g(1)
    tok.hand_off(gy)
    extra = tok.close()
    assert extra is gy and extra.data_ptr() == gy.data_ptr()
    assert tok.closed and tok.extra is None


def test_adopted_as_out_token():
    tok = GradToken()
    t = torch.ones(2, requires_grad=True) * 2
    assert not tok.adopted and not tok.produced(t)
    tok.adopt()
    assert tok.adopted and tok.produced(t)
    assert not tok.produced(t.detach())                  # nothing upstream requires a gradient: the plain branch
