"""Trainer.fit's host-side rules, without a GPU: the ModelCheckpoint(save_freq) counter (reference utils.py:128-132) and
the refusal of a validation stream that cannot be walked again (reference train.py:148-151)."""
import pytest

from x3d_tf_amd.train import SaveSchedule


def _saves(save_freq, epochs, steps, initial_epoch=0):
    """(global step, checkpoint number) of every write of a fit() call, replayed through SaveSchedule as fit() does."""
    s = SaveSchedule(save_freq)
    out, g = [], 0
    for e in range(initial_epoch, epochs):
        for _ in range(steps):
            g += 1
            n = s.after_batch(e)
            if n is not None:
                out.append((g, f"ckpt-{n}"))
        n = s.after_epoch(e)
        if n is not None:
            out.append((g, f"ckpt-{n}"))
    return out


def test_save_freq_counts_batches_across_epochs():
    # 2 epochs x 2 steps: the counter reaches 3 in the second epoch (index 1) and writes ckpt-2 there, never at epoch end
    assert _saves(3, 2, 2) == [(3, "ckpt-2")]
    assert _saves(1, 2, 2) == [(1, "ckpt-1"), (2, "ckpt-1"), (3, "ckpt-2"), (4, "ckpt-2")]
    assert _saves(2, 3, 3) == [(2, "ckpt-1"), (4, "ckpt-2"), (6, "ckpt-2"), (8, "ckpt-3")]
    assert _saves(5, 2, 2) == []


def test_save_freq_epoch_is_every_epoch_end():
    assert _saves("epoch", 2, 2) == [(2, "ckpt-1"), (4, "ckpt-2")]
    assert _saves("epoch", 4, 1, initial_epoch=2) == [(1, "ckpt-3"), (2, "ckpt-4")]


def test_save_freq_counter_starts_with_the_fit_call():
    # a resumed fit() (initial_epoch 1) counts its own batches: the 3rd is in epoch index 2
    assert _saves(3, 3, 2, initial_epoch=1) == [(3, "ckpt-3")]


@pytest.mark.parametrize("bad", [0, -2, 1.5, "steps", True, None])
def test_save_freq_refuses_other_values(bad):
    with pytest.raises(ValueError, match="save_freq"):
        SaveSchedule(bad)


def _dry_trainer():
    import x3d_tf_amd as x
    from x3d_tf_amd.model import X3D
    from x3d_tf_amd.train import Trainer
    cfg = x.get_config("XS", ["TRAIN.EPOCHS", 2])
    return Trainer(X3D(cfg, device="dry"), cfg)


class _NoBatches:
    """A training stream that fails the test if fit() takes a batch from it."""

    def __iter__(self):
        return self

    def __next__(self):
        raise AssertionError("fit() started training before refusing its arguments")


def test_one_shot_validation_iterator_is_refused_before_the_first_step():
    tr = _dry_trainer()
    one_shot = iter([("clips", "labels")])
    with pytest.raises(ValueError, match="callable"):
        tr.fit(_NoBatches(), epochs=2, steps_per_epoch=1, validation_data=one_shot)
    assert tr.epoch == 0
    # initial_epoch leaves two epochs to run: refused as well
    with pytest.raises(ValueError, match="callable"):
        tr.fit(_NoBatches(), epochs=3, steps_per_epoch=1, initial_epoch=1, validation_data=one_shot)


def test_fit_refuses_unknown_metrics_and_save_freq_before_the_first_step():
    tr = _dry_trainer()
    with pytest.raises(ValueError, match="metrics"):
        tr.fit(_NoBatches(), epochs=1, steps_per_epoch=1, metrics=("acc", "top_1_acc"))
    with pytest.raises(ValueError, match="save_freq"):
        tr.fit(_NoBatches(), epochs=1, steps_per_epoch=1, save_freq=0)
