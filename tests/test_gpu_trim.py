"""GPU: cpt_batch_extents and cpt_trim_batch through the C ABI -- the extents against cpt_amd/batching.py, the trimmed copies against
the torch slices bit for bit, into destination buffers filled with 0xFF and one guard row longer than what the launch may write."""
import numpy as np
import pytest
import torch

from cpt_amd import _lib as L
from cpt_amd import batching as BT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _extents(mask, Lt, pos, dev):
    m = torch.from_numpy(np.ascontiguousarray(mask)).to(dev)
    B, Lw = m.shape
    p = None if pos is None else torch.from_numpy(np.asarray(pos, np.int64)).to(dev)
    out = torch.full((4,), -7, dtype=torch.int32, device=dev)
    L.check(L.lib().cpt_batch_extents(m.data_ptr(), B, Lt, Lw - Lt, L.ptr(p), 0 if p is None else p.numel(), out.data_ptr(), L.stream_ptr()),
            "cpt_batch_extents")
    got = out.cpu().tolist()
    assert got[2:] == [-7, -7]                        # two int32 are written, no more
    return tuple(got[:2])


def _ragged_mask(B, Lt, Li, seed, holes=True):
    rng = np.random.Generator(np.random.PCG64(seed))
    m = np.zeros((B, Lt + Li), np.int64)
    for b in range(B):
        t, r = int(rng.integers(1, Lt + 1)), int(rng.integers(0, Li + 1))
        m[b, :t] = 1
        m[b, Lt:Lt + r] = 1
        if holes and t > 2:
            m[b, int(rng.integers(1, t - 1))] = 0
    return m


def test_extents_one_sequence(dev):
    for Lt, Li, t, r in ((7, 5, 3, 2), (7, 5, 7, 5), (1, 0, 1, 0), (165, 45, 23, 30), (9, 4, 0, 0)):
        m = np.zeros((1, Lt + Li), np.int64)
        m[0, :t] = 1
        m[0, Lt:Lt + r] = 1
        assert _extents(m, Lt, None, dev) == BT.batch_extent(m, Lt) == (max(t, 1), r)


def test_extents_tiny_shape_holes_empty_regions_last_slot(dev):
    Lt, Li = 7, 5                                     # the tiny golden's shape
    m = np.zeros((3, Lt + Li), np.int64)
    m[0, [0, 1, 4]] = 1                               # a hole at 2..3
    m[0, [Lt, Lt + 2]] = 1                            # and one among the regions
    m[1, :3] = 1
    m[2, :2] = 1
    assert _extents(m, Lt, None, dev) == BT.batch_extent(m, Lt) == (5, 3)
    no_regions = m.copy()
    no_regions[:, Lt:] = 0
    assert _extents(no_regions, Lt, None, dev) == (5, 0)                                  # Li' = 0
    last = m.copy()
    last[1, Lt - 1] = 1
    assert _extents(last, Lt, None, dev) == (7, 3)                                        # the last text slot set
    last[2, Lt + Li - 1] = 1
    assert _extents(last, Lt, None, dev) == (7, 5)
    # head rows: beyond the attended text, in the region part, outside the sequence; an odd element count (3 x 12 is even, 3 x 11 is not)
    for pos in ([1, 2, 0], [1, 6, 0], [0, 9, 0], [0, 0, 12], [-1, 0, 0]):
        assert _extents(m, Lt, pos, dev) == BT.batch_extent(m, Lt, np.array(pos)), pos
    odd = m[:, :Lt + Li - 1]
    assert _extents(odd, Lt, [1, 2, 0], dev) == BT.batch_extent(odd, Lt, np.array([1, 2, 0])) == (5, 3)
    # a mask that does not start on a 16-byte boundary takes the 8-byte path
    buf = torch.zeros(3 * (Lt + Li) + 1, dtype=torch.int64, device=dev)
    view = buf[1:].view(3, Lt + Li)
    view.copy_(torch.from_numpy(m))
    out = torch.zeros(2, dtype=torch.int32, device=dev)
    assert view.data_ptr() % 16 == 8
    L.check(L.lib().cpt_batch_extents(view.data_ptr(), 3, Lt, Li, None, 0, out.data_ptr(), L.stream_ptr()), "cpt_batch_extents")
    assert tuple(out.cpu().tolist()) == (5, 3)


@pytest.mark.parametrize("seed", [1, 2])
def test_extents_many_workgroups(dev, seed):
    B, Lt, Li = 300, 165, 45                          # 63000 entries: more than one workgroup's worth
    m = _ragged_mask(B, Lt, Li, seed)
    m[:, 150:165] = 0                                 # something is left to trim
    m[:, Lt + 40:] = 0
    want = BT.batch_extent(m, Lt)
    assert want[0] < Lt and want[1] < Li
    assert _extents(m, Lt, None, dev) == want
    pos = np.random.Generator(np.random.PCG64(seed)).integers(0, 160, B)
    assert _extents(m, Lt, pos, dev) == BT.batch_extent(m, Lt, pos)
    # the maximum sits in one entry only, anywhere in the batch
    for b, c in ((0, 164), (299, 164), (137, Lt + 44), (299, Lt + 44)):
        one = m.copy()
        one[b, c] = 1
        assert _extents(one, Lt, None, dev) == BT.batch_extent(one, Lt)


def test_extents_rejects_bad_arguments(dev):
    m = torch.ones((2, 5), dtype=torch.int64, device=dev)
    out = torch.zeros(2, dtype=torch.int32, device=dev)
    lib = L.lib()
    assert lib.cpt_batch_extents(None, 2, 3, 2, None, 0, out.data_ptr(), L.stream_ptr()) == -6
    assert lib.cpt_batch_extents(m.data_ptr(), 2, 0, 5, None, 0, out.data_ptr(), L.stream_ptr()) == -1
    assert lib.cpt_batch_extents(m.data_ptr(), 2, 3, 2, None, 2, out.data_ptr(), L.stream_ptr()) == -6      # positions announced, none given
    assert lib.cpt_trim_batch(m.data_ptr(), None, None, m.data_ptr(), None, 2, 3, 2, 4, 4, 0, m.data_ptr(), None, None, m.data_ptr(), None,
                              L.stream_ptr()) == -1                                                           # Lt_out > Lt
    assert lib.cpt_trim_batch(m.data_ptr(), None, None, m.data_ptr(), None, 2, 3, 2, 4, 2, 1, m.data_ptr(), None, None, m.data_ptr(), None,
                              L.stream_ptr()) == -6                                                           # regions kept, no features


def _poisoned(n, dtype, dev):
    """n elements of 0xFF bytes plus a guard row of 64 behind them that the launch must leave alone."""
    buf = torch.empty(n + 64, dtype=dtype, device=dev)
    buf.view(torch.uint8).fill_(0xFF)
    return buf


def _guard_intact(buf, n):
    return bool((buf[n:].view(torch.uint8) == 0xFF).all())


@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("D,B,Lt,Li,lt2,li2", [
    (38, 3, 7, 5, 5, 3),          # the tiny config
    (38, 3, 7, 5, 7, 0),          # Li' = 0: text untouched, no region copied
    (38, 3, 7, 5, 4, 5),          # Li' = Li
    (38, 2, 7, 5, 1, 1),
    (2054, 5, 165, 45, 23, 30),   # rows of 2054 floats start on 8-byte boundaries only
    (2054, 3, 70, 50, 40, 0),
    (2054, 3, 70, 50, 70, 50),    # nothing to cut: a plain copy
    (2054, 2, 12, 7, 12, 3),      # 3 x 2054 floats per sequence: the last chunk of a sequence is short (6162 = 4 x 1540 + 2)
    (37, 3, 9, 6, 4, 5),          # odd feature width: the scalar form
])
def test_trim_batch_equals_the_slices(dev, D, B, Lt, Li, lt2, li2, with_pos):
    g = torch.Generator().manual_seed(B * 1000 + D)
    ids = torch.randint(0, 30000, (B, Lt), generator=g).to(dev)
    tt = torch.randint(0, 2, (B, Lt), generator=g).to(dev)
    pos = torch.randint(0, 500, (B, Lt), generator=g).to(dev) if with_pos else None
    mask = torch.randint(0, 2, (B, Lt + Li), generator=g).to(dev)
    img = torch.randn((B, Li, D), generator=g).to(dev)
    n_t, n_m, n_f = B * lt2, B * (lt2 + li2), B * li2 * D
    ids_o, tt_o, mask_o = _poisoned(n_t, torch.int64, dev), _poisoned(n_t, torch.int64, dev), _poisoned(n_m, torch.int64, dev)
    pos_o = _poisoned(n_t, torch.int64, dev) if with_pos else None
    img_o = _poisoned(n_f, torch.float32, dev)
    L.check(L.lib().cpt_trim_batch(ids.data_ptr(), tt.data_ptr(), L.ptr(pos), mask.data_ptr(), img.data_ptr(), B, Lt, Li, D, lt2, li2,
                                   ids_o.data_ptr(), tt_o.data_ptr(), L.ptr(pos_o), mask_o.data_ptr(), img_o.data_ptr() if li2 else None,
                                   L.stream_ptr()), "cpt_trim_batch")
    torch.cuda.synchronize()
    assert torch.equal(ids_o[:n_t].view(B, lt2), ids[:, :lt2])
    assert torch.equal(tt_o[:n_t].view(B, lt2), tt[:, :lt2])
    if with_pos:
        assert torch.equal(pos_o[:n_t].view(B, lt2), pos[:, :lt2]) and _guard_intact(pos_o, n_t)
    assert torch.equal(mask_o[:n_m].view(B, lt2 + li2), torch.cat([mask[:, :lt2], mask[:, Lt:Lt + li2]], 1))
    # bit for bit: compared as integers, so that nothing hides behind a float comparison
    assert torch.equal(img_o[:n_f].view(torch.int32).view(B, li2, D), img[:, :li2].contiguous().view(torch.int32))
    assert _guard_intact(ids_o, n_t) and _guard_intact(tt_o, n_t) and _guard_intact(mask_o, n_m) and _guard_intact(img_o, n_f)


def test_trim_batch_without_token_types_and_unaligned_features(dev):
    """token_type is optional; a feature buffer that starts on a 4-byte boundary takes the scalar form."""
    B, Lt, Li, D, lt2, li2 = 3, 7, 5, 38, 4, 2
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, 500, (B, Lt), generator=g).to(dev)
    mask = torch.randint(0, 2, (B, Lt + Li), generator=g).to(dev)
    raw = torch.randn(B * Li * D + 1, generator=g).to(dev)
    img = raw[1:].view(B, Li, D)
    assert img.data_ptr() % 8 == 4
    ids_o, mask_o, img_o = _poisoned(B * lt2, torch.int64, dev), _poisoned(B * (lt2 + li2), torch.int64, dev), _poisoned(B * li2 * D, torch.float32, dev)
    L.check(L.lib().cpt_trim_batch(ids.data_ptr(), None, None, mask.data_ptr(), img.data_ptr(), B, Lt, Li, D, lt2, li2, ids_o.data_ptr(), None, None,
                                   mask_o.data_ptr(), img_o.data_ptr(), L.stream_ptr()), "cpt_trim_batch")
    torch.cuda.synchronize()
    assert torch.equal(ids_o[:B * lt2].view(B, lt2), ids[:, :lt2])
    assert torch.equal(mask_o[:B * (lt2 + li2)].view(B, lt2 + li2), torch.cat([mask[:, :lt2], mask[:, Lt:Lt + li2]], 1))
    assert torch.equal(img_o[:B * li2 * D].view(B, li2, D), img[:, :li2])
    assert _guard_intact(img_o, B * li2 * D) and _guard_intact(ids_o, B * lt2)
