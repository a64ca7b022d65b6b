"""dist.merge_draw_keys, the exchange of the sharded selectHost draw (include/yoda.h
yoda_shard_draw_keys): the elementwise UNSIGNED 64-bit MIN of the shards' keys.  torch has no
unsigned 64-bit MIN, so the keys travel as int64 with the sign bit flipped.  CPU tensors, the
local Reducer: no GPU."""
import numpy as np
import torch

from yoda_amd.dist import Reducer, ShardBuffers, merge_draw_keys

NONE = 2**64 - 1  # ~0: no key


def test_unsigned_min_over_three_shards():
    top = 1 << 63
    keys = np.array([
        # every shard ~0: ~0 survives
        [NONE, NONE, NONE],
        # one real key among ~0
        [NONE, 7, NONE],
        [NONE, NONE, top | 5],
        # bit 63 set against small: the small one is the unsigned minimum (signed MIN would
        # take the bit-63 value)
        [top | 1, 3, NONE],
        [(0xDEADBEEF << 32) | 70001, (0x7FFFFFFF << 32) | 12, (0x80000000 << 32) | 0],
        # all with bit 63 set
        [top | 9, top | 4, top | 6],
        # equal keys, zero, and the largest real key
        [42, 42, 42],
        [0, NONE, top],
        [NONE - 1, NONE, NONE],
    ], dtype=np.uint64).T.copy()  # [shard][pod]
    P = keys.shape[1]
    bufs = [ShardBuffers(P, torch.device("cpu")) for _ in range(3)]
    assert all(b.keys.dtype == torch.int64 and b.keys.numel() == P for b in bufs)
    for b, k in zip(bufs, keys):
        b.keys.copy_(torch.from_numpy(k.view(np.int64)))
    assert (bufs[0].keys[0] == -1).item()  # ~0 is -1 in the int64 view
    merge_draw_keys(Reducer(local=True), bufs)
    want = keys.min(axis=0)  # numpy's uint64 minimum
    for b in bufs:  # every shard holds the reduced keys
        np.testing.assert_array_equal(b.keys.numpy().view(np.uint64), want)
    every_none = (keys == np.uint64(NONE)).all(axis=0)
    np.testing.assert_array_equal(want == np.uint64(NONE), every_none)
    assert every_none.sum() == 1


def test_one_shard_is_the_identity():
    b = ShardBuffers(4, torch.device("cpu"))
    k = np.array([NONE, 1 << 63, 5, 0], np.uint64)
    b.keys.copy_(torch.from_numpy(k.view(np.int64)))
    merge_draw_keys(Reducer(local=True), [b])
    np.testing.assert_array_equal(b.keys.numpy().view(np.uint64), k)
