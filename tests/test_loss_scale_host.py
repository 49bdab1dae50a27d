"""CPU: the host rule of the dynamic loss scale (trainer.LossScaleControl: the arithmetic, the counters and the fixed-lag
queue) against optim_ref.loss_scale_ref, a plain loop over the flags written from the contract: the flag of step j is
applied at the start of step j + LAG, and what a step starts with depends on the flags of steps 0 .. i - LAG alone.

Everything here is exact: scales are powers of two between 1 and 65536, the rest are integers."""
import numpy as np
import pytest

import optim_ref as R

N = 64


def _run(flags, scale0, interval, dynamic=True, lag=None, read=int):
    """Drive the control the way Trainer.step does -- begin_step() first, the step's own flag pushed last -- and record what
    every step starts with.  -> (history, control)"""
    from object_detector_amd import trainer as T
    c = T.LossScaleControl(scale0, interval, dynamic, **({} if lag is None else {"lag": lag}), read=read)
    hist = []
    for f in flags:
        c.begin_step()
        hist.append(c.values())
        c.push(f)
    return hist, c


def _sequences():
    """(name, flags): the four shapes the control can go wrong on, then seeded random ones of every density."""
    yield "all clean", [0] * N
    yield "all bad", [1] * N
    yield "alternating", [i & 1 for i in range(N)]
    yield "alternating, bad first", [1 - (i & 1) for i in range(N)]
    for interval in (1, 2, 3):
        # a bad flag in place of the clean one that would double the scale, right behind that one, and one later
        for period in (interval, interval + 1, interval + 2):
            yield f"interval {interval}: a bad flag every {period}", [int(i % period == period - 1) for i in range(N)]
        yield f"one bad flag after {interval} clean ones", [0] * interval + [1] + [0] * (N - interval - 1)
    rng = np.random.default_rng(20)
    for k in range(300):
        p = (0.02, 0.1, 0.3, 0.5, 0.9)[k % 5]
        yield f"random {k} (p {p})", (rng.random(N) < p).astype(int).tolist()


SEQUENCES = list(_sequences())


def test_lag_and_limits_are_the_contract():
    from object_detector_amd import trainer as T
    assert T.LAG == 2 and (T.LOSS_SCALE_MIN, T.LOSS_SCALE_MAX) == (1.0, 65536.0)
    assert T.LossScaleControl(8.0).lag == 2 and T.LossScaleControl(8.0).interval == 2000


@pytest.mark.parametrize("interval", (1, 2, 3, 7))
@pytest.mark.parametrize("scale0", (1.0, 2.0, 256.0, 32768.0, 65536.0), ids=lambda s: f"scale{s:g}")
def test_history_is_the_reference(interval, scale0):
    """What every step starts with, over all the sequences, from a scale at the floor, next to it, in the middle, next to the
    cap and at the cap; and the drain at the end is the reference run LAG steps further with no new flags."""
    from object_detector_amd.trainer import LAG
    assert len(SEQUENCES) >= 300
    for name, flags in SEQUENCES:
        want = R.loss_scale_ref(flags, LAG, scale0, interval, steps=N + LAG)
        got, c = _run(flags, scale0, interval)
        assert got == want[:N], (name, next(i for i in range(N) if got[i] != want[i]))
        assert len(c.pending) == LAG
        assert c.pending_flags() == flags[-LAG:] and c.values() == got[-1]  # reading the pending flags applies none
        done = c.drain()
        assert done == flags[-LAG:] and not c.pending
        assert c.values() == want[N + LAG - 1], name
        assert c.skipped_steps == sum(flags)


def test_the_reference_itself_on_a_hand_worked_run():
    """interval 3, lag 2, bad flags at steps 2 and 5 of 8: worked by hand from the contract."""
    flags = [0, 0, 1, 0, 0, 1, 0, 0]
    want = [(64.0, 0, 0, 0),   # step 0: nothing applied
            (64.0, 0, 0, 0),   # step 1: nothing applied
            (64.0, 0, 1, 0),   # step 2: flag 0
            (64.0, 0, 2, 0),   # step 3: flag 1
            (32.0, 1, 0, 1),   # step 4: flag 2 is bad
            (32.0, 1, 1, 0),   # step 5: flag 3
            (32.0, 1, 2, 0),   # step 6: flag 4
            (16.0, 2, 0, 1),   # step 7: flag 5 is bad, one clean flag short of the doubling
            (16.0, 2, 1, 0),   # the run goes on with no new flags: flag 6
            (16.0, 2, 2, 0)]   # flag 7: everything applied
    assert R.loss_scale_ref(flags, 2, 64.0, 3, steps=10) == want
    assert R.loss_scale_ref(flags, 2, 64.0, 3) == want[:8]
    assert R.loss_scale_ref([0] * 7, 2, 64.0, 3)[-1] == (128.0, 0, 2, 0)  # flags 0 .. 4: doubled at the third, two more counted
    assert R.loss_scale_ref([0] * 4, 1, 64.0, 3)[3] == (128.0, 0, 0, 0)  # lag 1: step 3 starts with the flags of steps 0 .. 2 applied


@pytest.mark.parametrize("lag", (1, 2, 3, 5))
def test_other_lags_follow_the_same_rule(lag):
    for name, flags in SEQUENCES[::7]:
        got, c = _run(flags, 512.0, 2, lag=lag)
        assert got == R.loss_scale_ref(flags, lag, 512.0, 2), name
        c.drain()
        assert c.values() == R.loss_scale_ref(flags, lag, 512.0, 2, steps=N + lag)[-1], name


@pytest.mark.parametrize("bad", (1, -1, 0x100, 2, -(2 ** 31), 2 ** 31 - 1))
def test_any_nonzero_flag_is_bad(bad):
    from object_detector_amd.trainer import LAG
    rng = np.random.default_rng(3)
    ones = (rng.random(N) < 0.3).astype(int).tolist()
    flags = [f * bad for f in ones]
    got, c = _run(flags, 1024.0, 3)
    assert got == R.loss_scale_ref(flags, LAG, 1024.0, 3) == R.loss_scale_ref(ones, LAG, 1024.0, 3)
    assert got[-1][1] == sum(ones[:N - LAG]) > 0
    # the values arrive as numpy int32, as a pinned host flag's do
    got32, _ = _run([np.int32(f) for f in flags], 1024.0, 3)
    assert got32 == got


def test_fixed_scale_moves_the_counters_and_not_the_scale():
    from object_detector_amd.trainer import LAG
    for interval in (1, 2, 3):
        for name, flags in SEQUENCES[::5]:
            got, c = _run(flags, 512.0, interval, dynamic=False)
            assert got == R.loss_scale_ref(flags, LAG, 512.0, interval, dynamic=False), name
            assert all(h[0] == 512.0 for h in got)
            moving, _ = _run(flags, 512.0, interval)
            assert [h[1] for h in got] == [h[1] for h in moving] and [h[3] for h in got] == [h[3] for h in moving], name
            c.drain()
            assert c.loss_scale == 512.0 and c.skipped_steps == sum(flags)
    got, _ = _run([0, 1, 1, 0, 0, 0], 512.0, 1, dynamic=False)
    assert got[-1] == (512.0, 2, 1, 0)


def test_entries_are_read_once_when_applied_and_in_order():
    """The trainer's entries are not ints but (event, host flag) pairs its `read` waits for: begin_step() reads exactly the one
    entry it applies, the oldest, and returns it; nothing newer is touched."""
    from object_detector_amd.trainer import LAG, LossScaleControl
    reads = []

    def read(entry):
        reads.append(entry[0])
        return entry[1]
    flags = [0, 1, 0, 0, 1, 1, 0, 0, 0, 0]
    c = LossScaleControl(64.0, 3, read=read)
    for i, f in enumerate(flags):
        done = c.begin_step()
        assert done == ([(i - LAG, flags[i - LAG])] if i >= LAG else []) and reads == list(range(max(0, i - LAG + 1)))
        c.push((i, f))
    assert [e[0] for e in c.pending] == [8, 9]
    assert c.pending_flags() == [0, 0] and reads[-2:] == [8, 9] and len(c.pending) == 2
    assert c.values() == R.loss_scale_ref(flags, LAG, 64.0, 3)[-1]


def test_a_run_cut_in_two_with_the_pending_flags_carried_over(tmp_path):
    """What state_dict / save_state / load_state / load_state_dict do to the control: the values and the pending flags as an
    int32 array through an .npz, into a fresh control; the resumed history is the uninterrupted one at every cut."""
    from object_detector_amd import trainer as T, weights as W
    flags = SEQUENCES[-1][1]
    whole, _ = _run(flags, 256.0, 3)
    for cut in (0, 1, 2, 3, 17, N - 1):
        first, c = _run(flags[:cut], 256.0, 3)
        arr = np.array(c.pending_flags(), np.int32)
        assert arr.tolist() == flags[max(0, cut - T.LAG):cut]
        W.save_state(tmp_path / "s.npz", {"pending_flags": arr, "loss_scale": c.loss_scale, "_good_steps": c.good_steps,
                                          "skipped_steps": c.skipped_steps, "_consecutive_skips": c.consecutive_skips})
        sd = W.load_state(tmp_path / "s.npz")
        assert sd["pending_flags"].dtype == np.int32 and sd["pending_flags"].shape == (min(cut, T.LAG),)
        d = T.LossScaleControl(float(sd["loss_scale"]), 3)
        d.good_steps, d.skipped_steps, d.consecutive_skips = (int(sd[k]) for k in ("_good_steps", "skipped_steps", "_consecutive_skips"))
        d.pending[:] = [int(v) for v in sd["pending_flags"]]
        rest = []
        for f in flags[cut:]:
            d.begin_step()
            rest.append(d.values())
            d.push(f)
        assert first + rest == whole, cut
