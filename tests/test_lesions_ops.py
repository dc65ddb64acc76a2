"""pcms_component_table at the C ABI against predict.component_table, on the bytes: every column
is an integer (or a float picked by an integer key) combined by operations that commute, so there
is no tolerance and two runs must agree.  Table, header and workspace sit between guard bands;
header[0] (the status) must read 0 after every call on canonical labels.

The labels come from the host's label_components, so these cases test the table kernels alone.
A workgroup ranks 2048 consecutive voxels and a wave 512: 9x17x33 (5049 voxels) has three chunks
with a ragged end, 24x40x48 has 23, 1x1x257 half a wave's run, 1x1x1 one voxel."""
import numpy as np
import pytest
import torch

from tests.test_gpu_ops import DEV, _lib
from tests.test_lesions_host import BIG, SHAPES, _predict, labels, prob
from tests.test_predict_ops import _Guarded

pytestmark = pytest.mark.gpu

CASES = [("zeros", 26), ("ones", 26), ("checkerboard", 6), ("serpentine", 6)]
BERNOULLI_CASES = [("bernoulli6", 6), ("bernoulli18", 18), ("bernoulli26", 26)]
INT_MAX = 2 ** 31 - 1


def _packed_peaks(peak, index):
    bits = peak.view(np.uint32)
    key = bits ^ np.where(bits >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))
    return (key.astype(np.uint64) << np.uint64(32)) | (~index.view(np.uint32)).astype(np.uint64)


def _expected_bytes(table, capacity, with_prob):
    """The whole device table (include/pcms_hip.h has the layout) from the host table: its first
    min(K, capacity) rows, the initial values in the others."""
    k = min(len(table["label"]), capacity)
    index_sum = np.zeros((capacity, 3), np.int64)
    label, voxels = np.zeros(capacity, np.int32), np.zeros(capacity, np.int32)
    bbox = np.tile(np.array([INT_MAX, -1] * 3, np.int32), (capacity, 1))
    index_sum[:k], label[:k], voxels[:k], bbox[:k] = (table[c][:k] for c in ("index_sum", "label", "voxels", "bbox"))
    parts = [index_sum, label, voxels, bbox]
    if with_prob:
        packed, peak, index = np.zeros(capacity, np.uint64), np.zeros(capacity, np.float32), \
            np.full(capacity, -1, np.int32)
        packed[:k] = _packed_peaks(table["peak"][:k], table["peak_index"][:k])
        peak[:k], index[:k] = table["peak"][:k], table["peak_index"][:k]
        parts += [packed, peak, index]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def _buffers(shape, capacity, with_prob):
    L = _lib()
    nbytes = L.query("pcms_component_table_bytes", capacity, int(with_prob))
    nwork = L.query("pcms_component_table_work_bytes", *shape)
    assert nbytes == capacity * (72 if with_prob else 56) and nwork >= 4 * int(np.prod(shape)) and nwork % 4 == 0
    return (_Guarded(nbytes // 8, torch.int64, 0x5A5A5A5A5A5A5A5A), _Guarded(2, torch.int32, -7),
            _Guarded(nwork // 4, torch.int32, 0x5A5A5A5A))


def _device_table(lab, p, capacity):
    """(table bytes, status, K) of two runs on fresh buffers that agree."""
    L = _lib()
    dev = torch.from_numpy(np.ascontiguousarray(lab)).to(DEV)
    dp = None if p is None else torch.from_numpy(p).to(DEV)
    before = dev.clone()
    runs = []
    for _ in range(2):
        table, header, work = _buffers(lab.shape, capacity, p is not None)
        L.call("pcms_component_table", dev, dp, table.out, capacity, header.out, work.out, *lab.shape)
        work.check()
        h = header.check().numpy()
        runs.append((table.check().numpy().tobytes(), int(h[0]), int(h[1])))
    assert torch.equal(dev, before), "the labels were written"
    assert runs[0] == runs[1], "two runs differ"
    return runs[0]


def _check(lab, p, capacity):
    exp = _predict().component_table(lab, p)
    got, status, K = _device_table(lab, p, capacity)
    assert status == 0 and K == len(exp["label"])
    assert got == _expected_bytes(exp, capacity, p is not None)
    return K


@pytest.mark.parametrize("pattern,connectivity", CASES)
@pytest.mark.parametrize("shape", SHAPES)
def test_table_equals_host(shape, pattern, connectivity):
    lab = labels(pattern, shape, connectivity)
    K = len(np.unique(lab[lab > 0]))
    for p in (None, prob(shape)):
        assert _check(lab, p, K + 5) == K
        if K:
            _check(lab, p, K)  # exactly full


@pytest.mark.parametrize("pattern,connectivity", BERNOULLI_CASES)
@pytest.mark.parametrize("shape", BIG)
def test_table_equals_host_many_labels_per_wave(shape, pattern, connectivity):
    lab = labels(pattern, shape, connectivity)
    for p in (None, prob(shape), prob(shape, seed=1)):
        assert _check(lab, p, 4096) >= 100


@pytest.mark.parametrize("shape", BIG)
def test_a_table_smaller_than_the_component_count(shape):
    """n / 2 single-voxel components: the rows below capacity are exact, K is the true count and
    the guard band behind the table shows that no row past capacity was written."""
    lab = labels("checkerboard", shape, 6)
    K = (lab.size + 1) // 2
    for capacity in (1, 64, K - 1):
        for p in (None, prob(shape)):
            assert _check(lab, p, capacity) == K


def test_labels_that_are_not_canonical_set_the_status():
    """A label past the volume, INT_MAX, a negative one and one that names a background voxel: the
    bounds check skips the voxel and stores the status; the other rows are those of the volume
    without that voxel and no guard band is touched."""
    shape = (9, 17, 33)
    good = labels("bernoulli26", shape, 26)
    zero = np.flatnonzero(good.reshape(-1) == 0)
    at, other = int(zero[9]), int(zero[5])
    exp = _predict().component_table(good, prob(shape))
    for value in (good.size + 1, INT_MAX, -3, other + 1):
        bad = good.copy()
        bad.reshape(-1)[at] = value
        for p in (None, prob(shape)):
            got, status, K = _device_table(bad, p, 4096)
            assert status != 0 and K == len(exp["label"]), value
            assert got == _expected_bytes(exp, 4096, p is not None), value


def test_bad_arguments():
    L = _lib()
    lib = L.load()
    S = L.stream()
    shape = (3, 5, 7)
    n = int(np.prod(shape))
    lab = torch.zeros(n, dtype=torch.int32, device=DEV)
    p = torch.zeros(n, dtype=torch.float32, device=DEV)
    table, header, work = _buffers(shape, 16, True)
    lb, pp, tb, hd, wk = (t.data_ptr() for t in (lab, p, table.out, header.out, work.out))
    assert lib.pcms_component_table_work_bytes(0, 5, 7) < 0 and lib.pcms_component_table_work_bytes(3, -5, 7) < 0
    assert lib.pcms_component_table_work_bytes(1024, 1024, 1024) < 0  # 4 n bytes do not fit an int
    assert lib.pcms_component_table_bytes(0, 1) < 0 and lib.pcms_component_table_bytes(-4, 0) < 0
    assert lib.pcms_component_table_bytes(2 ** 30, 1) < 0
    for args in [(None, pp, tb, 16, hd, wk, *shape),        # NULL labels
                 (lb, pp, None, 16, hd, wk, *shape),        # NULL table
                 (lb, pp, tb, 16, None, wk, *shape),        # NULL header
                 (lb, pp, tb, 16, hd, None, *shape),        # NULL work
                 (lb + 2, pp, tb, 16, hd, wk, *shape),      # misaligned labels
                 (lb, pp + 1, tb, 16, hd, wk, *shape),      # misaligned prob
                 (lb, pp, tb + 4, 16, hd, wk, *shape),      # the table needs 8 bytes
                 (lb, pp, tb, 16, hd + 2, wk, *shape),      # misaligned header
                 (lb, pp, tb, 16, hd, wk + 1, *shape),      # misaligned work
                 (lb, pp, tb, 0, hd, wk, *shape),           # capacity < 1
                 (lb, pp, tb, -1, hd, wk, *shape),
                 (lb, pp, tb, 16, hd, wk, 0, 5, 7),         # a dimension < 1
                 (lb, pp, tb, 16, hd, wk, 3, -5, 7),
                 (lb, pp, tb, 16, hd, wk, 1024, 1024, 1024),  # past the workspace limit
                 (lb, pp, tb, 16, tb + 8, wk, *shape),      # header inside the table
                 (lb, pp, tb, 16, hd, tb + 16, *shape),     # work overlapping the table
                 (lb, pp, wk, 16, hd, wk, *shape),          # table aliasing work
                 (lb, pp, tb, 16, wk + 4, wk, *shape),      # header inside work
                 (tb, pp, tb, 16, hd, wk, *shape),          # labels aliasing the table
                 (lb, wk, tb, 16, hd, wk, *shape),          # prob aliasing work
                 (lb, None, tb, 16, wk, wk, *shape)]:       # ... also without prob
        assert lib.pcms_component_table(*args, S) < 0, args
    for g in (table, header, work):
        g.check(written=False)
    assert bool((lab == 0).all()) and bool((p == 0).all())
