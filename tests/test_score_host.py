"""CPU: the host side of model.score().  egomi_attn_suffix_shared is declared in include/egomi.h (so it is in the binder's table) and the
built library exports it; decode.candidate_lengths (first eos inclusive, else T; None counts all) agrees with a numpy restatement on eos at
0, in the middle, last, absent and twice; the driver accepts --rescore with its companions and refuses it without them."""
import ctypes

import numpy as np
import pytest
import torch

from egoscaler_amd import _abi, build as B, driver
from egoscaler_amd.decode import candidate_lengths


def test_suffix_entry_point_declared_and_exported():
    assert "egomi_attn_suffix_shared" in _abi.PROTOS
    ret, params = _abi.PROTOS["egomi_attn_suffix_shared"]
    own = _abi.PROTOS["egomi_attn_decode_shared"]
    assert ret is own[0] and [t for _, t in params] == [t for _, t in own[1]]      # the argument style of egomi_attn_decode_shared
    assert [n for n, _ in params][-4:] == ["T", "scale", "dtype", "stream"]
    assert hasattr(ctypes.CDLL(B.build()), "egomi_attn_suffix_shared")


def _lengths_np(cand, eos):
    out = np.full(cand.shape[:-1], cand.shape[-1], dtype=np.int32)
    if eos is None:
        return out
    for i in np.ndindex(*cand.shape[:-1]):
        hit = np.nonzero(cand[i] == eos)[0]
        if hit.size:
            out[i] = hit[0] + 1
    return out


def test_candidate_lengths_match_the_numpy_rule():
    eos, T = 2, 7
    rows = np.full((5, T), 9, dtype=np.int64)
    rows[0, 0] = eos                                                  # at 0
    rows[1, 3] = eos                                                  # in the middle
    rows[2, T - 1] = eos                                              # last
    rows[4, 2] = rows[4, 5] = eos                                     # twice (row 3: absent)
    want = np.array([1, 4, T, T, 3], dtype=np.int32)
    assert np.array_equal(_lengths_np(rows, eos), want)
    got = candidate_lengths(torch.from_numpy(rows), eos)
    assert got.dtype == torch.int32 and np.array_equal(got.numpy(), want)
    assert np.array_equal(candidate_lengths(torch.from_numpy(rows), None).numpy(), np.full(5, T, dtype=np.int32))
    rng = np.random.default_rng(0)
    for shape in ((3, 4, 9), (2, 1, 1), (6, 64)):
        cand = rng.integers(0, 4, size=shape).astype(np.int64)
        for e in (0, 3, 7, None):
            got = candidate_lengths(torch.from_numpy(cand), e)
            assert got.shape == cand.shape[:-1] and np.array_equal(got.numpy(), _lengths_np(cand, e)), (shape, e)


def test_driver_rescore_flag():
    base = ["eval", "--tiny"]
    assert driver.parse_args(base).rescore is False
    a = driver.parse_args(base + ["--num_samples", "4", "--select", "logprob", "--rescore"])
    assert a.rescore is True and a.num_samples == 4 and a.select == "logprob"
    for bad in (["--rescore"], ["--rescore", "--num_samples", "4"], ["--rescore", "--num_samples", "4", "--select", "medoid"],
                ["--rescore", "--select", "logprob"]):
        with pytest.raises(SystemExit):
            driver.parse_args(base + bad)
