"""LSTM training entry points and model plumbing without a GPU: argument validation on an unbound handle, the
training workspace size, the CPU model's refusal to compile and the flat-buffer layout (Keras weight order)."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def capi():
    from drnmf_amd import _capi
    _capi.lib()
    return _capi


def _arr(*ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def test_train_entry_points_validate_without_a_gpu(capi):
    from drnmf_amd import ops
    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.drnmf_create_unbound(ctypes.byref(h)) == 0
    try:
        fake = ctypes.c_void_p(0x100000)                 # never dereferenced: validation fails first
        good = ops.make_lstm_desc(4, 10, 33, 13, 2)
        need = L.drnmf_lstm_train_workspace_bytes(ctypes.byref(good))
        assert need > L.drnmf_lstm_workspace_bytes(ctypes.byref(good))
        ptrs = _arr(0x100000, 0x100000)

        def fwd(d, ws_bytes=need, x=fake, ld=16, ws=fake):
            return L.drnmf_lstm_train_forward(h, d, x, -1.0, fake, fake, ld, ws, ws_bytes, None)

        def head(d, ws_bytes=need, y=fake, ld=16):
            return L.drnmf_lstm_loss_head_backward(h, d, y, fake, fake, ld, fake, fake, fake, fake, fake, fake, fake,
                                                   ws_bytes, None)

        def bwd(d, ws_bytes=need, dk=ptrs, dh=fake):
            return L.drnmf_lstm_backward(h, d, ptrs, ptrs, dh, dk, ptrs, ptrs, fake, ws_bytes, None)

        for field, v in (("B", 0), ("T", -1), ("F", 0), ("H", 0), ("K", 0), ("recurrent_activation", 99)):
            d = ops.make_lstm_desc(4, 10, 33, 13, 2)
            setattr(d, field, v)
            assert fwd(ctypes.byref(d)) == -1
            assert head(ctypes.byref(d)) == -1
            assert bwd(ctypes.byref(d)) == -1
            assert L.drnmf_lstm_train_workspace_bytes(ctypes.byref(d)) == (0 if field != "recurrent_activation"
                                                                           else need)
        g = ctypes.byref(good)
        assert fwd(None) == -1 and head(None) == -1 and bwd(None) == -1
        assert fwd(g, need - 1) == -4 and head(g, need - 1) == -4 and bwd(g, need - 1) == -4   # DRNMF_ERR_WORKSPACE
        assert b"workspace" in L.drnmf_last_error(h)
        assert fwd(g, x=None) == -1 and fwd(g, ws=None) == -1
        assert head(g, y=None) == -1 and bwd(g, dh=None) == -1
        assert bwd(g, dk=_arr(0x100000, None)) == -1       # a NULL inside the pointer arrays
        assert fwd(g, ld=12) == -1 and head(g, ld=12) == -1  # row stride ld_h < H
        assert fwd(g, ws=ctypes.c_void_p(0x100010)) == -1    # misaligned workspace
    finally:
        L.drnmf_destroy(h)


def test_train_workspace_grows_with_batch_and_frames(capi):
    from drnmf_amd import ops
    L = capi.lib()
    size = lambda B, T: L.drnmf_lstm_train_workspace_bytes(ctypes.byref(ops.make_lstm_desc(B, T, 513, 250, 5)))
    assert 0 < size(1, 10) < size(2, 10) < size(2, 20)
    assert size(32, 500) < size(32, 1000)
    d = ops.make_lstm_desc(4, 10, 33, 13, 2)           # the inference sizes are those of the inference layout
    assert L.drnmf_lstm_workspace_bytes(ctypes.byref(d)) < L.drnmf_lstm_train_workspace_bytes(ctypes.byref(d))


def test_cpu_model_still_refuses_compile_and_flat_layout_is_keras_order():
    from drnmf_amd import layers
    m = layers.build_lstm(dict(mask_value=-1., maxseq=8, input_dim=7, output_dim=7, K_layers=2, hidden_dim=5),
                          device="cpu")
    with pytest.raises(NotImplementedError):
        m.compile(lr=1e-4, clipnorm=1.0)
    items = m.flat_layout_items()
    names = [n for n, _ in items]
    l0, l1, dense = m.lstms[0].name, m.lstms[1].name, m.dense.name
    assert names == [l0 + "/kernel:0", l0 + "/recurrent_kernel:0", l0 + "/bias:0",
                     l1 + "/kernel:0", l1 + "/recurrent_kernel:0", l1 + "/bias:0",
                     dense + "/kernel:0", dense + "/bias:0"]
    sizes = [int(t.numel()) for _, t in items]
    assert sizes == [7 * 20, 5 * 20, 20, 5 * 20, 5 * 20, 20, 5 * 7, 7]
    assert all(a is b for (_, a), b in zip(items, m.weights))      # the same tensors, in get_weights order
    offsets = np.cumsum([0] + sizes)
    assert offsets[-1] == sum(w.size for w in m.get_weights())
