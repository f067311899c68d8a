"""CPU-side pin of the STFT family's argument checks (csrc/stft.hip, csrc/stft_stream.h): which code and which
message an entry answers a bad FFT size with, which of two faults wins, and the frame-count rule.  Every call runs
on a drnmf_create_unbound handle with fake pointers that are never dereferenced, and none has all-valid arguments
(the one exception is refused for the unbound handle), so nothing is enqueued (no GPU needed)."""
import ctypes

import pytest

INVALID, UNSUPPORTED, HIP, WORKSPACE = -1, -2, -3, -4
BAD_N = (0, 32, 48, 500, 8192, -512)
SIZES = [(512, 128), (1024, 256), (64, 16), (512, 512)]      # tests/test_stream_host.py
FAKE = ctypes.c_void_p(0x100000)
BIG = 1 << 30


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import _capi
    return _capi.lib()


@pytest.fixture()
def handle(lib):
    h = ctypes.c_void_p()
    assert lib.drnmf_create_unbound(ctypes.byref(h)) == 0
    yield h
    lib.drnmf_destroy(h)


# ---- the entries: a call with valid defaults, every argument a keyword ------------------------------------------
def stft_mag(L, h, n_sig=2, nsampl=1000, N=512, hop=128, pcm=FAKE, mag=FAKE):
    return L.drnmf_stft_mag(h, n_sig, nsampl, N, hop, 1, pcm, mag, None)


def stft(L, h, n_sig=2, nsampl=1000, N=512, hop=128, pcm=FAKE, re=FAKE, im=FAKE):
    return L.drnmf_stft(h, n_sig, nsampl, N, hop, 1, pcm, re, im, None, None)


def istft_masked(L, h, n_sig=2, n_frames=8, nsampl=1000, N=512, hop=128, re=FAKE, nb=BIG):
    return L.drnmf_istft_masked(h, n_sig, n_frames, nsampl, N, hop, re, FAKE, FAKE, FAKE, FAKE, nb, None)


def stft_ragged(L, h, n_sig=3, b=2, N=512, hop=128, pcm=FAKE):
    return L.drnmf_stft_ragged(h, n_sig, 1001, FAKE, b, FAKE, 32, N, hop, 1, -1.0, pcm, FAKE, FAKE, FAKE, None)


def istft_ragged(L, h, b=2, N=64, hop=16, re=FAKE, ld=33, nb=BIG):          # N = 64: the workspace pair
    return L.drnmf_istft_ragged(h, 3, b, 32, N, hop, FAKE, FAKE, re, FAKE, FAKE, ld, FAKE, 1024, 0, FAKE, nb, None)


def stft_pair_chunks(L, h, n_sig=3, stride_y=1000, n_seq=4, N=512, hop=128, transform=0, x=FAKE):
    return L.drnmf_stft_pair_chunks(h, n_sig, 1200, stride_y, FAKE, FAKE, n_seq, FAKE, 16, N, hop, 1, transform,
                                    -1.0, FAKE, FAKE, x, FAKE, FAKE, None)


def stft_pair_chunks_target(L, h, n_sig=3, stride_y=1000, n_seq=4, N=512, hop=128, transform=0, target=1, x=FAKE):
    return L.drnmf_stft_pair_chunks_target(h, n_sig, 1200, stride_y, FAKE, FAKE, n_seq, FAKE, 16, N, hop, 1,
                                           transform, target, -1.0, FAKE, FAKE, x, FAKE, FAKE, None)


def stft_pair_frames(L, h, n_sig=3, stride_y=1000, total_frames=40, N=512, hop=128, transform=0, x=FAKE):
    return L.drnmf_stft_pair_frames(h, n_sig, 1200, stride_y, FAKE, FAKE, FAKE, total_frames, N, hop, 1, transform,
                                    FAKE, FAKE, x, FAKE, None)


def stream_reset(L, h, B=3, N=512, hop=128, state=FAKE, nb=BIG):
    return L.drnmf_stream_reset(h, B, N, hop, state, nb, None)


def stream_forward(L, h, B=3, T=8, N=512, hop=128, chunk=FAKE, state=FAKE, nb=BIG):
    return L.drnmf_stream_forward(h, B, 1000, T, N, hop, 1, -1.0, chunk, FAKE, FAKE, FAKE, FAKE, FAKE, state, nb,
                                  None)


def stream_inverse(L, h, B=3, T=8, N=512, hop=128, re=FAKE, ld=257, state=FAKE, nb=BIG):
    return L.drnmf_stream_inverse(h, B, T, N, hop, re, FAKE, FAKE, ld, 1, 0, FAKE, 1024, state, nb, None)


# ---- the faults of an entry in the order it checks them: (arguments, code, message, the message is complete) ----
def size_fault(who, code, N=48):
    return (dict(N=N), code, "%s: N=%d must be a power of two in [64,4096]" % (who, N), True)


OVERFLOW = dict(stride_y=1 << 31, hop=1)      # 2^31 + N + 2 frames at hop 1


def pair_faults(who):                         # check_stft_pair's, behind the entry's own first check
    return [(dict(n_sig=0), INVALID, who + ": bad shape n_sig=0 ", False),
            size_fault(who, INVALID),
            (dict(transform=7), INVALID, who + ": transform=7 is neither", False),
            (OVERFLOW, INVALID, who + ": stride_y=2147483648 at hop=1 has more than", False),
            (dict(x=None), INVALID, who + ": NULL pointer argument", True)]


def stream_faults(who):                       # check_stream's
    return [(dict(B=0), INVALID, who + ": B=0 must lie in", False),
            size_fault(who, INVALID),
            (dict(hop=96), INVALID, who + ": hop=96 must divide", False),
            (dict(state=None), INVALID, who + ": NULL state", True),
            (dict(nb=100), INVALID, who + ": state of 100 bytes is below", False)]


CHUNKS_T = "stft_pair_chunks_target"
ENTRIES = {
    "stft_mag": (stft_mag, UNSUPPORTED, [
        (dict(n_sig=0), INVALID, "stft_mag: bad shape", False),
        size_fault("stft_mag", UNSUPPORTED),
        (dict(pcm=None), INVALID, "stft_mag: NULL pointer argument", True)]),
    "stft": (stft, UNSUPPORTED, [
        (dict(n_sig=0), INVALID, "stft: bad argument", True),
        size_fault("stft", UNSUPPORTED)]),
    "stft/NULL": (stft, UNSUPPORTED, [
        (dict(re=None), INVALID, "stft: bad argument", True),
        size_fault("stft", UNSUPPORTED)]),
    "istft_masked": (istft_masked, UNSUPPORTED, [
        (dict(re=None), INVALID, "istft_masked: bad argument", True),
        size_fault("istft_masked", UNSUPPORTED),
        (dict(nb=100), WORKSPACE, "istft_masked: workspace too small", True)]),
    "stft_ragged": (stft_ragged, INVALID, [
        (dict(b=65536), INVALID, "stft_ragged: bad shape", False),
        size_fault("stft_ragged", INVALID),
        (dict(pcm=None), INVALID, "stft_ragged: NULL pointer argument", True)]),
    "istft_ragged": (istft_ragged, INVALID, [
        (dict(b=0), INVALID, "istft_ragged: bad shape", False),
        size_fault("istft_ragged", INVALID),
        (dict(re=None), INVALID, "istft_ragged: NULL pointer argument", True),
        (dict(ld=32), INVALID, "istft_ragged: ld_mask=32 is below", False),
        (dict(nb=100), WORKSPACE, "istft_ragged: workspace too small", False)]),
    "stft_pair_chunks": (stft_pair_chunks, INVALID, [
        (dict(n_seq=0), INVALID, "stft_pair_chunks: bad shape n_seq=0 ", False)] + pair_faults("stft_pair_chunks")),
    CHUNKS_T: (stft_pair_chunks_target, INVALID, [
        (dict(target=7), INVALID, CHUNKS_T + ": target=7 is none of", False),
        (dict(n_seq=0), INVALID, CHUNKS_T + ": bad shape n_seq=0 ", False)] + pair_faults(CHUNKS_T) + [
        (dict(transform=1), INVALID, CHUNKS_T + ": target=1 is defined for", False),
        (dict(), HIP, CHUNKS_T + ": the handle is bound to no device", True)]),
    "stft_pair_frames": (stft_pair_frames, INVALID, [
        (dict(total_frames=0), INVALID, "stft_pair_frames: bad shape total_frames=0", False)] +
        pair_faults("stft_pair_frames")),
    "stream_reset": (stream_reset, INVALID, stream_faults("stream_reset")),
    "stream_forward": (stream_forward, INVALID, [
        (dict(T=0), INVALID, "stream_forward: bad shape", False),
        (dict(chunk=None), INVALID, "stream_forward: NULL pointer argument", True)] +
        stream_faults("stream_forward")),
    "stream_inverse": (stream_inverse, INVALID, [
        (dict(T=0), INVALID, "stream_inverse: bad shape", False),
        (dict(re=None), INVALID, "stream_inverse: NULL pointer argument", True)] +
        stream_faults("stream_inverse") + [
        (dict(ld=256), INVALID, "stream_inverse: ld_mask=256 is below", False)]),
}


def expect(L, h, fn, kw, code, text, whole):
    assert L.drnmf_snr(h, 0, 1, FAKE, FAKE, FAKE, None) == INVALID      # leaves another entry's message
    assert fn(L, h, **kw) == code, (fn.__name__, kw)
    msg = L.drnmf_last_error(h).decode()
    assert msg == text if whole else msg.startswith(text), (fn.__name__, kw, msg)


@pytest.mark.parametrize("name", [n for n in ENTRIES if n != "stft/NULL"])
def test_size_faults(lib, handle, name):
    fn, code, _ = ENTRIES[name]
    who = fn.__name__
    hop = dict(hop=1) if who.startswith("stream") else {}        # a hop that the stream entries' N % hop admits
    for N in BAD_N:
        expect(lib, handle, fn, dict(N=N, **hop), code, "%s: N=%d must be a power of two in [64,4096]" % (who, N),
               True)
        assert lib.drnmf_stream_state_bytes(3, N, 1) == 0
        assert lib.drnmf_stream_state_bytes(3, N, 128) == 0
    assert fn(lib, None, N=48) == INVALID                        # no handle: nowhere to leave a message


@pytest.mark.parametrize("name", list(ENTRIES))
def test_the_first_of_two_faults_wins(lib, handle, name):
    fn, _, faults = ENTRIES[name]
    for kw, code, text, whole in faults:                         # every fault alone ...
        expect(lib, handle, fn, kw, code, text, whole)
    for (kw0, code, text, whole), (kw1, _, _, _) in zip(faults, faults[1:]):     # ... and with the next one
        assert not set(kw0) & set(kw1), (name, kw0, kw1)
        expect(lib, handle, fn, dict(kw0, **kw1), code, text, whole)


@pytest.mark.parametrize("N,hop", SIZES)
def test_frame_counts(lib, N, hop):
    f, s = ctypes.c_int64(), ctypes.c_int64()
    for n in (0, 1, hop - 1, hop, hop + 1, 3 * hop + 7, 16001):
        nf = 1 + (-(-n // hop) * hop + N) // hop
        assert lib.drnmf_stft_frames(n, N, hop) == nf
        for crop in (0, 1):
            assert lib.drnmf_stream_counts(n, 1, N, hop, crop, ctypes.byref(f), ctypes.byref(s)) == 0
            # closed: the offline frames, and istft_mc's trim of N on both sides (cropped to the input)
            assert (f.value, s.value) == (nf, min(n, hop * (nf - 1) - N) if crop else hop * (nf - 1) - N)
            assert lib.drnmf_stream_counts(n, 0, N, hop, crop, ctypes.byref(f), ctypes.byref(s)) == 0
            # open: the frames whose last sample has arrived, and the samples no coming frame reaches
            assert (f.value, s.value) == (n // hop + 1, max(0, (n // hop + 1) * hop - N))
    assert lib.drnmf_stft_frames(-1, N, hop) == -1
    assert lib.drnmf_stft_frames(10, 0, hop) == -1
    assert lib.drnmf_stft_frames(10, N, 0) == -1
