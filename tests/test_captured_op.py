"""device.CapturedOp off the GPU: nothing is captured, no agreement call is made, the operator stays eager."""
import torch


def test_cpu_device_stays_eager_and_never_agrees():
    from sem_amd.device import CapturedOp
    calls = []

    def agree(ok):
        calls.append(ok)
        return True

    fn = lambda v: 3.0 * v - 1.0   # noqa: E731
    op = CapturedOp("cpu", fn, 257, agree=agree, seed=5)
    assert op.graph is None and op.x is None and op.out is None
    assert calls == []
    v = torch.rand(257, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    keep = v.clone()
    assert torch.equal(op(v), fn(v)) and torch.equal(v, keep)
    assert calls == []
