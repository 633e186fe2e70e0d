"""tests/redzone.py on CPU tensors: the layout arithmetic, the alignments, and that check() catches what it is for."""
import numpy as np
import pytest
import torch

import redzone


@pytest.mark.parametrize("dtype,aligns", [(torch.float64, (0, 8, 16, 248)), (torch.float32, redzone.F32_OFFSETS),
                                          (torch.int64, (0,)), (torch.uint8, (0, 1))])
@pytest.mark.parametrize("n", [1, 3, 1000, (1 << 20) - 1, 1 << 20])
def test_layout(n, dtype, aligns):
    for al in aligns:
        data = None if dtype == torch.float64 and n % 2 else torch.ones(n, dtype=dtype)
        g = redzone.guarded(n, dtype, al, data=data, role="out" if data is None else "in", poison=(7 if dtype == torch.int64 else None),
                            device="cpu", name="v")
        if data is None:
            g.t.fill_(2)
        assert g.t.numel() == n and g.t.dtype == dtype
        assert g.t.data_ptr() % 256 == al
        front = g.t.data_ptr() - g.buf.data_ptr()
        back = g.buf.data_ptr() + g.buf.numel() - (g.t.data_ptr() + n * g.es)
        want = (1 << 20) if n >= (1 << 20) else (64 << 10)
        assert want <= front < want + 512 and want <= back < want + 1024
        assert g.a is not None and g.a.ctypes.data == g.t.data_ptr()
        g.check()


def test_poison_values():
    assert abs(redzone.poison_value(torch.float64) - 10001.29) < 0.01
    assert abs(redzone.poison_value(torch.float32) - 10001.41) < 0.01
    assert redzone.poison_value(torch.int64, 3000) == 1000
    assert redzone.poison_value(torch.uint8) == 1
    g = redzone.guarded(5, torch.float64, 8, role="out", device="cpu")
    assert np.all(g.buf[: g.start].view(torch.float64).numpy() == redzone.poison_value(torch.float64))
    assert g.t.view(torch.int64)[0].item() == redzone.POISON_F64


@pytest.mark.parametrize("dtype,al", [(torch.float64, 0), (torch.float64, 8), (torch.float32, 4), (torch.float32, 12)])
def test_check_catches_each_fault(dtype, al):
    n = 100
    x = torch.arange(n, dtype=dtype)

    def out():
        g = redzone.guarded(n, dtype, al, role="out", device="cpu", name="y")
        g.t.copy_(x)
        return g

    whole = lambda g: g.buf.view(dtype)
    first = lambda g: g.start // g.es  # index of interior element 0 in the whole buffer
    g = out()
    g.check()
    # one element in front of the interior
    whole(g)[first(g) - 1] = 0
    with pytest.raises(AssertionError, match=r"y: front guard written at element offset -1 "):
        g.check()
    # one element behind it
    g = out()
    whole(g)[first(g) + n] = 0
    with pytest.raises(AssertionError, match=r"y: back guard written at element offset %d " % n):
        g.check()
    # far behind it, inside the guard band
    g = out()
    whole(g)[first(g) + n + 5000 // g.es] = 0
    with pytest.raises(AssertionError, match="back guard"):
        g.check()
    # an unwritten interior element
    g = redzone.guarded(n, dtype, al, role="out", device="cpu", name="y")
    g.t[: n - 1].copy_(x[: n - 1])
    with pytest.raises(AssertionError, match=r"y: interior element %d still holds the poison \(1 unwritten\)" % (n - 1)):
        g.check()
    # a modified read-only input
    q = redzone.guarded(n, dtype, al, data=x, device="cpu", name="q")
    q.check()
    q.t[37] = -1
    with pytest.raises(AssertionError, match=r"q: read-only input changed at interior element 37"):
        q.check()
    # ... which an in-out buffer (y aliasing q) may be
    yq = redzone.guarded(n, dtype, al, data=x, role="inout", device="cpu", name="yq")
    yq.t[37] = -1
    yq.check()
    whole(yq)[yq.start // yq.es + n] = 0
    with pytest.raises(AssertionError, match="yq: back guard"):
        yq.check()


def test_masks_and_indices():
    m = redzone.guarded(10, torch.uint8, 0, role="out", device="cpu", name="mask")
    assert int(m.t[0]) == redzone.POISON_U8_OUT and int(m.buf[0]) == redzone.POISON_U8_OUT
    m.t.fill_(1)
    m.check()
    z = redzone.Zone(device="cpu")
    off = z.add(4, torch.int64, data=torch.tensor([0, 3, 5, 9]), poison=3, name="offsets")
    z.add(9, torch.uint8, data=torch.ones(9, dtype=torch.uint8), name="sel")
    assert int(off.buf.view(torch.int64)[0]) == 3
    z.check()
    off.buf.view(torch.int64)[off.end // 8] = 0
    with pytest.raises(AssertionError, match="offsets: back guard written at element offset 4"):
        z.check()


def test_modes():
    assert set(redzone.F64_MODES) == {"A", "B", "C", "D"}
    for k, (ay, ai) in redzone.F64_MODES.items():
        assert ay % 8 == 0 and ai % 8 == 0


def test_set_input_moves_the_snapshot_with_the_element():
    """an input element the test rewrites itself passes check(); the same element written behind the helper's back does not"""
    x = np.arange(7, dtype=np.float32)
    g = redzone.guarded(7, torch.float32, 12, data=x, device="cpu", name="x")
    g.set_input(3, 2.5)
    assert g.a[3] == np.float32(2.5)
    g.check()
    g.t[3] = 1.0
    with pytest.raises(AssertionError, match="read-only input changed at interior element 3"):
        g.check()
