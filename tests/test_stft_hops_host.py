"""CPU-side tests of the transform grid at hops other than N/4 (tests/stft_hops_ref.py): the frame and sample
counts of the C ABI and of ops against an actual oracle run at every size and length, the branch of csrc/stft.hip
each size takes (so the grid cannot silently stop covering what it claims), and the streaming counts at the hops
that divide N and their refusal at the hops that do not (no GPU needed)."""
import numpy as np
import pytest

import stft_hops_ref as R
from oracle import drnmf_oracle as O


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import _capi
    return _capi


def test_the_grid_is_the_one_written_down():
    assert len(R.SIZES) == 16 and len(set(R.SIZES)) == 16
    assert R.lengths(512, 160) == [1, 159, 160, 161, 487, 9999, 16001]
    assert R.lengths(512, 8) == [1, 7, 8, 9, 31, 3000]                  # capped at 3000
    assert R.lengths(4096, 1024) == [1, 1023, 1024, 1025, 3079, 2 * 4096 + 5]
    assert R.lengths(64, 64)[:2] == [1, 63]
    for N, hop in R.SIZES:
        lens = R.lengths(N, hop)
        assert min(lens) >= 1 and len(set(lens)) == len(lens)
        assert set(R.equal_lengths(N, hop)) <= set(lens)
        _, pcm = R.signals(N, hop, True)
        assert pcm.shape[1] % 2 == 1 and pcm.shape[1] > max(lens)       # odd stride, junk behind every length
    for sub in (R.INDEPENDENCE_SIZES, R.T_CUT_SIZES, R.PAIR_SIZES):
        assert set(sub) <= set(R.SIZES)
    assert all(N % hop == 0 for N, hop in R.STREAM_SIZES)
    # with 9999 and 16001 every fused size crosses at least four run boundaries
    for N, hop in R.FUSED:
        if (N, hop) != (512, 8):
            assert R.out_length(9999, N, hop) > 4 * R.fused_run(hop)
    assert R.out_length(3000, 512, 8) > R.fused_run(8)                  # (512, 8): one boundary under its cap


@pytest.mark.parametrize("N,hop", R.SIZES, ids=R.ids(R.SIZES))
def test_counts_equal_an_actual_oracle_run(capi, N, hop):
    from drnmf_amd import ops
    L = capi.lib()
    lens = R.lengths(N, hop)
    S, full = R.spectra(N, hop, False), R.reconstructions(N, hop, False)
    for i, n in enumerate(lens):
        nf = S[i].shape[1]
        assert S[i].shape[0] == N // 2 + 1
        assert nf == O.stft_frames(n, N, hop) == ops.stft_frames(n, N, hop) == L.drnmf_stft_frames(n, N, hop) \
            == R.frames(n, N, hop)
        cropped = R.reconstruct(S[i], None, N, hop, nsampl=n)
        n_full, n_crop = full[i].shape[0], cropped.shape[0]
        assert n_full == int(ops.ragged_out_lengths([n], N, hop)[0]) == R.out_length(n, N, hop)
        assert n_crop == int(ops.ragged_out_lengths([n], N, hop, True)[0]) == R.out_length(n, N, hop, True)
        assert n_full == hop * (nf - 1) - N and n_crop == min(n, n_full)
        # no length of the grid reaches an empty output
        assert n_full >= 1
        if hop <= N:
            assert n_full == -(-n // hop) * hop - N % hop >= hop - N % hop > 0
            assert (n_full % hop == 0) == (N % hop == 0)                # not a multiple of a hop that does not divide N
    both = ops.ragged_out_lengths(lens, N, hop)
    assert [int(v) for v in both] == [r.shape[0] for r in full]


@pytest.mark.parametrize("N,hop", R.SIZES, ids=R.ids(R.SIZES))
def test_every_size_takes_the_branch_the_grid_claims(capi, N, hop):
    """The ragged inverse is fused exactly where drnmf_istft_ragged_workspace_bytes is 0; the forward path is fast
    exactly at N = 512 / 1024 (stft_fast in csrc/stft.hip, which the fused inverse presupposes)."""
    L = capi.lib()
    fwd, inv, _ = R.GRID[(N, hop)]
    assert fwd in ("fast", "general") and inv in ("fused", "two-stage")
    assert (fwd == "fast") == (N in (512, 1024))
    for b, T in ((1, 1), (3, 7), (5, 131)):
        got = L.drnmf_istft_ragged_workspace_bytes(b, T, N, hop)
        assert got == (0 if inv == "fused" else b * T * N * 4), (b, T, got)
    assert (inv == "fused") == (fwd == "fast" and hop <= N)
    # fft_lds runs wherever the fast bodies do not: its odd-log2 first stage at N = 128, 2048 and at (512, 600)
    log2 = N.bit_length() - 1
    assert 1 << log2 == N
    reaches_odd_stage = (log2 & 1) == 1 and (fwd == "general" or inv == "two-stage")
    assert reaches_odd_stage == ((N, hop) in [(512, 600), (128, 32), (128, 64), (2048, 512)])
    assert (4096 + 2048) * 8 == 48 * 1024 and (2048 + 1024) * 8 == 24 * 1024      # the dynamic LDS of the table


def test_what_the_fused_sizes_add():
    assert R.FUSED == [(512, 256), (1024, 512), (512, 512), (512, 160), (512, 129), (512, 8), (1024, 1000)]
    assert R.fused_run(160) == 1920 and R.fused_run(1000) == 2000 and R.fused_run(129) == 15 * 129
    assert all(R.fused_run(h) == 2048 for h in (256, 512, 8))
    assert 2048 // 1000 == 2                                            # C = 2
    # frames over a sample: N / hop where the hop divides N
    assert (512 // 256, 512 // 512, 512 // 8) == (2, 1, 64)
    # an odd hop alternates the parity of a frame's first sample, an even one never changes it
    assert [(f * 129 - 512) % 2 for f in range(4, 8)] == [0, 1, 0, 1]
    assert all(hop % 2 == 0 for N, hop in R.SIZES if N in (512, 1024) and hop not in (129, 1025))
    # hop > N leaves hop - N samples per hop under no frame
    for N, hop in R.HOP_ABOVE_N:
        n_out = R.out_length(16001, N, hop)
        u = R.uncovered(n_out, N, hop)
        assert int(u.sum()) == (hop - N) * -(-16001 // hop) > 0
        ref = R.reconstructions(N, hop, True)[-1]
        assert ref.shape[0] == n_out and np.all(ref[u] == 0.0) and np.any(ref[~u] != 0.0)


@pytest.mark.parametrize("N,hop", R.DIVIDING, ids=R.ids(R.DIVIDING))
def test_stream_counts_of_a_closed_stream(capi, N, hop):
    from drnmf_amd import ops
    S, full = R.spectra(N, hop, False), R.reconstructions(N, hop, False)
    for i, n in enumerate(R.lengths(N, hop)):
        assert ops.stream_counts(n, True, N, hop) == (S[i].shape[1], full[i].shape[0])
        assert ops.stream_counts(n, True, N, hop, crop=True) == (S[i].shape[1], min(n, full[i].shape[0]))


def test_streaming_refuses_the_hops_that_do_not_divide_N(capi):
    from drnmf_amd import ops
    L = capi.lib()
    bad = [s for s in R.SIZES if s not in R.DIVIDING]
    assert set(bad) == {(512, 160), (512, 129), (1024, 1000), (512, 600), (1024, 1025), (256, 96), (64, 100)}
    for N, hop in bad:
        for closed in (False, True):
            with pytest.raises(ValueError):
                ops.stream_counts(1000, closed, N, hop)
        assert L.drnmf_stream_state_bytes(1, N, hop) == 0
        with pytest.raises(ValueError):
            ops.stream_state(1, N, hop, "cpu")                          # refused before anything is allocated
    for N, hop in R.STREAM_SIZES:
        assert L.drnmf_stream_state_bytes(1, N, hop) > 0
