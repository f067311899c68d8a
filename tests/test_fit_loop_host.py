"""The epoch loop of fit() and fit_waveform() on CPU fakes, no GPU: which batches are taken in which order, which
callback events fire around them and with which logs, when a loss is waited for, and what the history holds.  Every
expected value is a literal, recorded from the loops as they stood before they were folded into one."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def layers():
    import __graft_entry__ as G
    G.build()
    from drnmf_amd import layers
    return layers


class _Loss(object):
    """What a step returns: a number that counts how often, and where in the event stream, it is waited for."""

    def __init__(self, value, events):
        self.value, self.events, self.floats = float(value), events, 0

    def __float__(self):
        self.floats += 1
        self.events.append(("float", self.value))
        return self.value


class _AllEvents(object):
    """A callback with all five events; stop_at: the epoch whose on_epoch_end sets model.stop_training."""

    def __init__(self, events, stop_at=None):
        self.events, self.stop_at = events, stop_at

    def on_train_begin(self, logs=None):
        self.events.append(("train_begin",))

    def on_epoch_begin(self, ep, logs=None):
        self.events.append(("epoch_begin", ep))

    def on_batch_end(self, i, logs=None):
        self.events.append(("batch_end", i, logs["batch"], logs["size"], logs["loss"]))

    def on_epoch_end(self, ep, logs=None):
        self.events.append(("epoch_end", ep, dict(logs)))
        if ep == self.stop_at:
            self.model.stop_training = True

    def on_train_end(self, logs=None):
        self.events.append(("train_end",))


def _no_floats(events):
    return [e for e in events if e[0] != "float"]


def _fit_fake(layers, events):
    class Fake(layers._SequenceModel):
        """train_on_batch records (first feature of every row as ints, live) and returns the length of the event
        stream behind that record (waits not counted); _validate records a call and returns 0.5."""

        def __init__(self):
            self.weights_seen = []
            self.losses = []

        def _device(self):
            return "cpu"

        def _stateful(self):
            return False

        def train_on_batch(self, x, y, sample_weight=None, _live=True):
            events.append(("step", [int(v) for v in x[:, 0, 0]], _live))
            self.weights_seen.append(sample_weight)
            self.losses.append(_Loss(len(_no_floats(events)), events))
            return self.losses[-1]

        def _validate(self, validation_data, batch_size, take):
            events.append(("validate",))
            return 0.5
    return Fake()


def _data():
    x = np.empty((5, 3, 2), np.float32)
    for i in range(5):
        x[i] = i
    return x, np.ones((5, 3), np.float32)


def test_fit_event_stream_and_history(layers):
    ev = []
    x, w = _data()
    hist = _fit_fake(layers, ev).fit(x, x, sample_weight=w, batch_size=2, epochs=4, seed=3, validation_data=(x, x),
                                     callbacks=[_AllEvents(ev, stop_at=1)])
    assert _no_floats(ev) == [
        ("train_begin",),
        ("epoch_begin", 0),
        ("step", [3, 4], True), ("batch_end", 0, 0, 2, 3.0),
        ("step", [1, 0], True), ("batch_end", 1, 1, 2, 5.0),
        ("step", [2], True), ("batch_end", 2, 2, 1, 7.0),
        ("validate",),
        ("epoch_end", 0, {"loss": 5.0, "val_loss": 0.5}),
        ("epoch_begin", 1),
        ("step", [2, 1], True), ("batch_end", 0, 0, 2, 12.0),
        ("step", [3, 4], True), ("batch_end", 1, 1, 2, 14.0),
        ("step", [0], True), ("batch_end", 2, 2, 1, 16.0),
        ("validate",),
        ("epoch_end", 1, {"loss": 14.0, "val_loss": 0.5}),
        ("train_end",),
    ]
    assert hist == {"loss": [5.0, 14.0], "val_loss": [0.5, 0.5]}


def test_fit_without_shuffle_takes_input_order_and_no_validation_leaves_val_loss_empty(layers):
    ev = []
    x, w = _data()
    model = _fit_fake(layers, ev)
    hist = model.fit(x, x, sample_weight=w, batch_size=2, epochs=2, shuffle=False, callbacks=[_AllEvents(ev)])
    assert _no_floats(ev) == [
        ("train_begin",),
        ("epoch_begin", 0),
        ("step", [0, 1], True), ("batch_end", 0, 0, 2, 3.0),
        ("step", [2, 3], True), ("batch_end", 1, 1, 2, 5.0),
        ("step", [4], True), ("batch_end", 2, 2, 1, 7.0),
        ("epoch_end", 0, {"loss": 5.0}),
        ("epoch_begin", 1),
        ("step", [0, 1], True), ("batch_end", 0, 0, 2, 11.0),
        ("step", [2, 3], True), ("batch_end", 1, 1, 2, 13.0),
        ("step", [4], True), ("batch_end", 2, 2, 1, 15.0),
        ("epoch_end", 1, {"loss": 13.0}),
        ("train_end",),
    ]
    assert hist == {"loss": [5.0, 13.0], "val_loss": []}
    assert all(sw.shape == (len(b[1]), 3) and (sw == 1).all()
               for sw, b in zip(model.weights_seen, [e for e in ev if e[0] == "step"]))
    assert model.stop_training is False


def test_no_loss_is_waited_for_before_the_epoch_ends_without_a_batch_callback(layers):
    ev = []
    x, w = _data()

    class EpochOnly(object):
        def on_epoch_end(self, ep, logs=None):
            ev.append(("epoch_end", ep, dict(logs)))

    model = _fit_fake(layers, ev)
    hist = model.fit(x, x, sample_weight=w, batch_size=2, epochs=2, seed=3, callbacks=[EpochOnly()])
    assert ev == [
        ("step", [3, 4], True), ("step", [1, 0], True), ("step", [2], True),
        ("float", 1.0), ("float", 2.0), ("float", 3.0),
        ("epoch_end", 0, {"loss": 2.0}),
        ("step", [2, 1], True), ("step", [3, 4], True), ("step", [0], True),
        ("float", 5.0), ("float", 6.0), ("float", 7.0),
        ("epoch_end", 1, {"loss": 6.0}),
    ]
    assert [l.floats for l in model.losses] == [1] * 6
    assert hist == {"loss": [2.0, 6.0], "val_loss": []}
    # with a batch callback every step's loss is waited for at once, and once more for the epoch's mean
    ev2 = []
    model = _fit_fake(layers, ev2)
    model.fit(x, x, sample_weight=w, batch_size=2, epochs=1, seed=3, callbacks=[_AllEvents(ev2)])
    assert [e[0] for e in ev2] == ["train_begin", "epoch_begin"] + ["step", "float", "batch_end"] * 3 + \
        ["float"] * 3 + ["epoch_end", "train_end"]
    assert [l.floats for l in model.losses] == [2] * 3


def test_callbacks_are_bound_by_set_model_or_by_attribute(layers):
    x, w = _data()

    class WithSetModel(object):
        got = None

        def set_model(self, model):
            self.got = model

    class Plain(object):
        pass

    a, b = WithSetModel(), Plain()
    model = _fit_fake(layers, [])
    model.fit(x, x, sample_weight=w, batch_size=5, epochs=1, callbacks=[a, b])
    assert a.got is model and not hasattr(a, "model")
    assert b.model is model


def test_a_rank_that_has_run_out_replays_its_first_batch_with_zero_weights(layers, monkeypatch):
    from drnmf_amd import dp
    # one step more than this rank has batches; the empty-shard question (0 here) is left alone
    monkeypatch.setattr(dp, "max_over_ranks", lambda v: int(v) + 1 if v else int(v))
    ev = []
    x, w = _data()
    model = _fit_fake(layers, ev)
    hist = model.fit(x, x, sample_weight=w, batch_size=2, epochs=2, seed=3)
    assert [e for e in ev if e[0] == "step"] == [
        ("step", [3, 4], True), ("step", [1, 0], True), ("step", [2], True), ("step", [3, 4], False),
        ("step", [2, 1], True), ("step", [3, 4], True), ("step", [0], True), ("step", [2, 1], False),
    ]
    for i, sw in enumerate(model.weights_seen):
        if i in (3, 7):
            assert isinstance(sw, np.ndarray) and sw.dtype == np.float32 and sw.shape == (2, 3) and not sw.any()
        else:
            assert (sw == 1).all()
    assert hist == {"loss": [2.5, 6.5], "val_loss": []}


def test_an_empty_shard_is_refused_before_the_first_step(layers):
    ev = []
    x, w = _data()
    with pytest.raises(ValueError, match=r"fit\(\): a rank holds no sequences \(0 here\)"):
        _fit_fake(layers, ev).fit(x[:0], x[:0], sample_weight=w[:0], batch_size=2, callbacks=[_AllEvents(ev)])
    assert ev == [("train_begin",)]


def test_pretrain_fit_unwraps_the_doubled_targets_and_weights(layers):
    ev = []
    x, w = _data()

    class Fake(layers.SNMFCostPretrainModel):
        def __init__(self):
            self.seen = []

        def _device(self):
            return "cpu"

        def _stateful(self):
            return False

        def train_on_batch(self, x, y=None, sample_weight=None, _live=True):
            self.seen.append((x, y, sample_weight))
            return _Loss(len(self.seen), ev)

        def _validate(self, validation_data, batch_size, take):
            self.val = validation_data
            return 0.25

    model = Fake()
    hist = model.fit(x, [x, x], sample_weight=[w, w], validation_data=(x, [x, x], [w, w]), batch_size=2, epochs=1,
                     shuffle=False)
    assert len(model.seen) == 3
    for (xb, yb, wb), rows in zip(model.seen, ([0, 1], [2, 3], [4])):
        assert isinstance(yb, np.ndarray) and isinstance(wb, np.ndarray)
        assert np.array_equal(xb, x[rows]) and np.array_equal(yb, x[rows]) and np.array_equal(wb, w[rows])
    assert len(model.val) == 3 and model.val[0] is x and model.val[1] is x and model.val[2] is w
    assert hist == {"loss": [2.0], "val_loss": [0.25]}
    # y left out: the input is the target
    model = Fake()
    model.fit(x, sample_weight=[w, w], batch_size=5, epochs=1, shuffle=False)
    assert np.array_equal(model.seen[0][1], x)


def _wave_fake(layers, events):
    import torch

    class Fake(layers._SequenceModel):
        """The waveform loop's collaborators, each recording its call: a bank of n 'recordings', batches that
        name their rows, a flat buffer on the CPU and a step that returns the length of the event stream."""
        mask_value = -1.0
        _flat = None

        def __init__(self):
            self.losses = []

        def _device(self):
            return "cpu"

        def _input_width(self):
            return 33

        def _wave_bank(self, noisy, clean, N, hop, max_samples, what):
            events.append(("bank", len(noisy), N, hop, max_samples, what))
            return None, None, None, np.array([len(v) for v in noisy], dtype=np.int64)

        def _wave_batch(self, bank, b, N, hop, kind):
            events.append(("batch", [int(i) for i in b], N, hop, kind))
            return [int(i) for i in b], "cot_fn"

        def loss_and_grads_cot(self, x, cot_fn, live=True):
            events.append(("grads", x, cot_fn, live))
            return torch.zeros(4)

        def apply_gradients(self, flat):
            events.append(("adam", tuple(flat.shape)))
            self.losses.append(_Loss(len(_no_floats(events)), events))
            return self.losses[-1]
    return Fake()


def test_fit_waveform_event_stream_and_history(layers):
    ev = []
    wavs = [np.zeros(100 + i, np.float32) for i in range(5)]
    model = _wave_fake(layers, ev)
    hist = model.fit_waveform(wavs, wavs, loss="wave_mse", batch_size=2, epochs=4, seed=0, N=64, hop=16,
                              callbacks=[_AllEvents(ev, stop_at=1)])
    assert _no_floats(ev) == [
        ("bank", 5, 64, 16, None, "fit_waveform"),
        ("train_begin",),
        ("epoch_begin", 0),
        ("batch", [2, 0], 64, 16, "wave_mse"), ("grads", [2, 0], "cot_fn", True), ("adam", (4,)),
        ("batch_end", 0, 0, 2, 6.0),
        ("batch", [1, 3], 64, 16, "wave_mse"), ("grads", [1, 3], "cot_fn", True), ("adam", (4,)),
        ("batch_end", 1, 1, 2, 10.0),
        ("batch", [4], 64, 16, "wave_mse"), ("grads", [4], "cot_fn", True), ("adam", (4,)),
        ("batch_end", 2, 2, 1, 14.0),
        ("epoch_end", 0, {"loss": 10.0}),
        ("epoch_begin", 1),
        ("batch", [0, 2], 64, 16, "wave_mse"), ("grads", [0, 2], "cot_fn", True), ("adam", (4,)),
        ("batch_end", 0, 0, 2, 20.0),
        ("batch", [1, 4], 64, 16, "wave_mse"), ("grads", [1, 4], "cot_fn", True), ("adam", (4,)),
        ("batch_end", 1, 1, 2, 24.0),
        ("batch", [3], 64, 16, "wave_mse"), ("grads", [3], "cot_fn", True), ("adam", (4,)),
        ("batch_end", 2, 2, 1, 28.0),
        ("epoch_end", 1, {"loss": 24.0}),
        ("train_end",),
    ]
    assert hist == {"loss": [10.0, 24.0], "val_loss": []}
    assert [l.floats for l in model.losses] == [2] * 6


def test_fit_waveform_replays_with_live_false_and_waits_only_at_the_epoch_end(layers, monkeypatch):
    from drnmf_amd import dp
    monkeypatch.setattr(dp, "max_over_ranks", lambda v: int(v) + 1 if v else int(v))
    ev = []
    wavs = [np.zeros(100 + i, np.float32) for i in range(3)]
    model = _wave_fake(layers, ev)
    hist = model.fit_waveform(wavs, wavs, batch_size=2, epochs=1, shuffle=False, N=64, hop=16)
    assert [e[1:] for e in ev if e[0] == "grads"] == [([0, 1], "cot_fn", True), ([2], "cot_fn", True),
                                                      ([0, 1], "cot_fn", False)]
    assert [e[0] for e in ev][-3:] == ["float"] * 3 and [l.floats for l in model.losses] == [1] * 3
    assert hist == {"loss": [7.0], "val_loss": []}
