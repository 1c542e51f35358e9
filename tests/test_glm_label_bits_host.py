"""``ops.glm.pack_labels_torch``, the host twin of the label pack kernel, against a plain loop."""
import numpy as np
import pytest
import torch

from orange3_spark_amd.ops import glm as G


@pytest.mark.parametrize("n", [0, 15, 16, 17, 4097])
def test_pack_twin_matches_a_plain_loop(n):
    rng = np.random.default_rng(n + 1)
    y = (rng.random(n) < 0.5).astype(np.float32)
    words, bad = G.pack_labels_torch(torch.from_numpy(y))
    ref = np.zeros(n // 16, dtype=np.int32)
    for t in range(n // 16):
        for j in range(16):
            if y[16 * t + j] == 1.0:
                ref[t] |= 1 << j
    assert not bad
    assert words.dtype == torch.int32 and words.shape == (n // 16,)
    assert np.array_equal(words.numpy(), ref)


@pytest.mark.parametrize("value", [0.5, float("nan"), -0.0])
def test_pack_twin_flags_what_is_neither_0_nor_1(value):
    y = torch.tensor([0.0, 1.0] * 16)
    assert not G.pack_labels_torch(y)[1]
    y[21] = value
    words, bad = G.pack_labels_torch(y)
    assert bad
    assert words.shape == (2,)
    # beyond the last whole tile nothing is packed and nothing counts
    y2 = torch.tensor([1.0] * 16 + [value])
    words, bad = G.pack_labels_torch(y2)
    assert not bad and words.tolist() == [0xFFFF]
