"""device.CapturedOp on one GPU with no process group: the capture order, the agreement protocol (a recording stub in
the place of parallel.all_agree) and the replay, on 257 doubles and elementwise torch arithmetic."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 257


def fn(v):
    return 3.0 * v * v - 0.5 * v + 1.0


class Agree:
    """agree(ok): records ok and returns the next of `answers` (None: ok itself, as a one-rank MIN all-reduce)."""

    def __init__(self, *answers):
        self.calls, self.answers = [], list(answers)

    def __call__(self, ok):
        self.calls.append(ok)
        a = self.answers.pop(0) if self.answers else None
        return ok if a is None else a


def fresh(gpu, seed=3):
    return torch.rand(N, dtype=torch.float64, device=gpu, generator=torch.Generator(device=gpu).manual_seed(seed))


def test_agreed_capture_replays_bitwise(gpu):
    from sem_amd.device import CapturedOp
    agree = Agree()
    op = CapturedOp(gpu, fn, N, agree=agree, seed=5)
    assert agree.calls == [True, True]
    assert op.graph is not None and op.x.shape == (N,) and op.out.shape == (N,)
    v = fresh(gpu)
    keep = v.clone()
    assert torch.equal(op(v), fn(v))
    assert torch.equal(v, keep)


def test_first_agreement_refused_drops_the_graph(gpu):
    from sem_amd.device import CapturedOp
    agree = Agree(False)
    op = CapturedOp(gpu, fn, N, agree=agree, seed=5)
    assert agree.calls == [True]           # no second agreement call
    assert op.graph is None and op.out is None
    v = fresh(gpu)
    assert torch.equal(op(v), fn(v))       # eager


def test_replay_that_differs_from_the_warm_up_drops_the_graph(gpu):
    from sem_amd.device import CapturedOp
    count = [0]

    def drifting(v):       # the counter's value is a constant of the captured launch: the replay adds 2, the warm-up 1
        count[0] += 1
        return fn(v) + float(count[0])

    agree = Agree()
    op = CapturedOp(gpu, drifting, N, agree=agree, seed=5)
    assert agree.calls == [True, False]
    assert op.graph is None and op.out is None
    assert torch.equal(op(fresh(gpu)), fn(fresh(gpu)) + 3.0)     # eager: the third invocation
    assert count[0] == 3


def test_capture_that_raises_reports_no_and_leaves_the_device_usable(gpu):
    from sem_amd.device import CapturedOp
    count = [0]

    def refusing(v):       # a plain Python error on the second invocation, which is the one inside the capture
        count[0] += 1
        y = fn(v)
        if count[0] == 2:
            raise RuntimeError("refused inside the capture")
        return y

    agree = Agree()
    op = CapturedOp(gpu, refusing, N, agree=agree, seed=5)
    assert agree.calls == [False]
    assert op.graph is None and op.out is None
    v = fresh(gpu)
    got = op(v)            # eager, on a device that still works
    assert count[0] == 3 and torch.equal(got, fn(v))
    # against the host's arithmetic: five roundings of 2^-53 relative each on intermediates below 4
    assert (got.cpu() - fn(v.cpu())).abs().max().item() <= 5 * 4 * 2.0 ** -53


def test_no_agree_uses_the_graph_as_captured(gpu):
    from sem_amd.device import CapturedOp
    op = CapturedOp(gpu, fn, N)
    assert op.graph is not None
    v = fresh(gpu)
    assert torch.equal(op(v), fn(v))
