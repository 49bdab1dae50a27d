"""GPU: the loss-scale control's schedule does not depend on timing.  The flag of step j is applied at the start of step j + 2 --
never earlier, never later -- so what a step starts with (loss_scale, skipped_steps, _good_steps, _consecutive_skips, and with
them diverged()) is optim_ref.loss_scale_ref of the flags of the steps up to two back, whether the host waits for the device
after every step or runs as far ahead as it can, whether or not state_dict() was called, however fit() is cut into calls, and
across a resume from a state file.

Real steps at 2 x 96^2 on weights.random_init(2), run in pieces (loss_scale_sched.run_steps) so that an Inf can be put into a
step's loss gradient; buffers are compared whole and bit for bit.
"""
import numpy as np
import pytest
import torch

import loss_scale_sched as L
import optim_ref as R

pytestmark = pytest.mark.gpu

B, S = 2, 96
SCALE0 = 256.0
BUFFERS = ("params", "mom", "run_stats")


@pytest.fixture(scope="module")
def setup(cuda):
    from test_gpu_trainer_update import _setup
    params, x, anns = _setup()
    return params, torch.from_numpy(x).to(cuda), anns


def _trainer(cuda, params, **kw):
    from object_detector_amd.trainer import Trainer
    tr = Trainer(params, B, (S, S), device=cuda, **dict(dict(lr=0.01, momentum=0.9, weight_decay=1e-4, loss_scale=SCALE0), **kw))
    tr.loss_scale_growth_interval = L.INTERVAL
    return tr


def _target(tr, anns):
    return tr.pb.encode_batch(anns, return_device=True)[0]


def _same_buffers(a, b, what):
    for k in BUFFERS:
        assert torch.equal(getattr(a, k).view(torch.int32), getattr(b, k).view(torch.int32)), f"{what}: {k} differs"


@pytest.fixture(scope="module")
def spin(cuda, setup):
    """(cycles of the lazy twin's spin, measured ms per step, ticks per ms): SPIN_STEPS times one step of this configuration."""
    params, xt, anns = setup
    tr = _trainer(cuda, params)
    ms = L.measure_step_ms(tr, xt, _target(tr, anns))
    rate = L.ticks_per_ms()
    print(f"one step at {B} x {S}^2: {ms:.2f} ms; spin {L.SPIN_STEPS * ms:.1f} ms = {int(L.SPIN_STEPS * ms * rate)} ticks")
    return int(L.SPIN_STEPS * ms * rate), ms, rate


@pytest.fixture(scope="module")
def eager(cuda, setup):
    """The 8 steps with an Inf at steps 2 and 5 and the host waiting for the device after every step: the trainer afterwards
    (nothing drained), what every step started with, the device flags.  Shared; nobody steps it further."""
    params, xt, anns = setup
    tr = _trainer(cuda, params)
    hist, flags = L.run_steps(tr, xt, _target(tr, anns), 8, inject=L.INJECT, eager=True)
    return tr, hist, flags.cpu().tolist()


def test_timing_twins_follow_one_schedule(cuda, setup, eager, spin):
    """An eager twin (torch.cuda.synchronize() after every step: every flag has landed when the next step begins) and a lazy
    twin (a spin kernel between allreduce() and sgd(): the step's flag copy is still in flight when the next step begins, and
    the device falls further behind with every step) start every step with the same control values, those of the reference,
    and end with the same bits in params, mom and run_stats.

    Measured on an MI355X: one step of this configuration takes 5.57 ms (host launches included); the spin is SPIN_STEPS = 4
    steps long, 22.3 ms = 51.4 M ticks of a clock measured at 2.31 M ticks/ms.  The test measures both again on every run
    (the `spin` fixture) and prints them.

    Where the scale changes by a power of two the parameters do not notice (exact in f16 and f32 away from the subnormal and
    overflow ends), so a control that applied a flag at another step shows in the histories, not in the buffers."""
    params, xt, anns = setup
    cycles, ms, _rate = spin
    etr, ehist, eflags = eager
    ltr = _trainer(cuda, params)
    lhist, lflags = L.run_steps(ltr, xt, _target(ltr, anns), 8, inject=L.INJECT, spin=cycles)
    lflags = lflags.cpu().tolist()
    want = R.loss_scale_ref(L.FLAGS, L.LAG, SCALE0, L.INTERVAL, steps=8 + L.LAG)
    print("eager", ehist, "\nlazy ", lhist, "\nref  ", want[:8])
    assert eflags == L.FLAGS and lflags == L.FLAGS, "the injected Inf did not reach the device flag"
    assert ehist == want[:8], "eager twin"
    assert lhist == want[:8], "lazy twin"
    assert want[4][0] == SCALE0 / 2 and want[3][0] == SCALE0  # the flag of step 2 is applied at step 4, not at step 3
    _same_buffers(etr, ltr, "eager and lazy twin")
    assert len(ltr._flag_queue) == L.LAG  # nothing newer than step i - 2 was applied
    ltr._poll_nonfinite(wait=True)
    assert L.control(ltr) == want[8 + L.LAG - 1] and ltr.skipped_steps == 2


def test_state_dict_is_an_observer(cuda, setup, eager):
    """state_dict() after steps 3 and 4, thrown away: the run goes on as if it had not been called."""
    params, xt, anns = setup
    etr, ehist, eflags = eager
    tr = _trainer(cuda, params)
    seen = []

    def observe(i):
        if i in (3, 4):
            seen.append(tr.state_dict()["pending_flags"].tolist())
    hist, flags = L.run_steps(tr, xt, _target(tr, anns), 8, inject=L.INJECT, after_step=observe)
    assert flags.cpu().tolist() == eflags == L.FLAGS
    assert seen == [L.FLAGS[2:4], L.FLAGS[3:5]]
    assert hist == ehist
    _same_buffers(tr, etr, "with and without state_dict()")
    assert tr.pending_flags() == etr.pending_flags() == L.FLAGS[6:]


def test_fit_in_pieces_is_fit_in_one(cuda, setup):
    """fit() for 8 steps and as 3 + 5: buffers, control values (read when fit() asks the schedule for each step's learning rate,
    and at the end) and the loss history are the same; neither drains."""
    params, xt, anns = setup
    runs = []
    for pieces in ((8,), (3, 5)):
        tr = _trainer(cuda, params)
        y = _target(tr, anns)
        seen = []

        def schedule(step):
            seen.append((step, L.control(tr)))
            return 0.01

        def batches():
            while True:
                yield xt, y
        feed, hists, done = batches(), [], 0
        for k in pieces:
            hists.append(tr.fit(feed, k, lr_schedule=schedule, start_step=done))
            done += k
        runs.append((tr, seen, np.concatenate(hists)))
    (one, seen1, hist1), (two, seen2, hist2) = runs
    want = R.loss_scale_ref([0] * 8, L.LAG, SCALE0, L.INTERVAL, steps=9)
    # the schedule is asked BEFORE the step applies its flag: step i sees what step i - 1 started with
    assert seen1 == [(i, want[max(i - 1, 0)]) for i in range(8)]
    assert seen2 == seen1
    assert L.control(one) == L.control(two) == want[7] and want[7][0] == 4 * SCALE0
    assert len(one._flag_queue) == len(two._flag_queue) == L.LAG
    assert hist1.shape == (8, 4) and hist1.tobytes() == hist2.tobytes()
    _same_buffers(one, two, "fit(8) and fit(3) + fit(5)")


def test_resume_with_a_bad_flag_pending(cuda, setup, tmp_path):
    """An Inf at step 3, the state taken right after step 3 -- its flag is pending, [0, 1] with step 2's -- through
    save_state / load_state into a trainer built from other weights: the 5 steps that follow start with the control values
    and end with the buffers of the uninterrupted 9-step run, step by step.  The same state without the array is the older
    format: it loads with nothing pending."""
    from object_detector_amd import weights as W
    params, xt, anns = setup
    tr = _trainer(cuda, params)
    y = _target(tr, anns)
    snaps, states = {}, []

    def after(i):
        if i == 3:
            states.append(tr.state_dict())
        if i >= 4:
            snaps[i] = {k: getattr(tr, k).clone() for k in BUFFERS}
    hist, flags = L.run_steps(tr, xt, y, 9, inject=(3,), after_step=after)
    bad3 = [0, 0, 0, 1, 0, 0, 0, 0, 0]
    assert flags.cpu().tolist() == bad3
    want = R.loss_scale_ref(bad3, L.LAG, SCALE0, L.INTERVAL)
    assert hist == want and want[5][0] == want[4][0] / 2  # doubled at step 4 (flags 0 .. 2), halved at step 5 (flag 3)
    sd = states[0]
    assert sd["pending_flags"].dtype == np.int32 and sd["pending_flags"].tolist() == [0, 1]
    assert (sd["loss_scale"], sd["skipped_steps"], sd["_good_steps"], sd["_consecutive_skips"]) == want[3]
    W.save_state(tmp_path / "state.npz", sd)
    loaded = W.load_state(tmp_path / "state.npz")
    assert loaded["pending_flags"].dtype == np.int32 and loaded["pending_flags"].tolist() == [0, 1]

    from test_gpu_trainer_update import _setup
    other = _trainer(cuda, _setup(seed=7)[0], loss_scale=32.0)
    L.run_steps(other, xt, y, 1, inject=(0,))  # a flag of its own in flight: the loaded state replaces it
    other.load_state_dict(loaded)
    assert other.pending_flags() == [0, 1] and L.control(other) == want[3]

    def compare(i):
        for k in BUFFERS:
            assert torch.equal(getattr(other, k).view(torch.int32), snaps[i][k].view(torch.int32)), f"after step {i}: {k}"
    rest, _ = L.run_steps(other, xt, y, 5, after_step=compare, first=4)
    assert rest == want[4:], "the resumed run applies the pending flags at other steps than the uninterrupted run"
    assert other.pending_flags() == tr.pending_flags() == [0, 0]
    snaps.clear()

    old = {k: v for k, v in loaded.items() if k != "pending_flags"}
    other.load_state_dict(old)
    assert not other._flag_queue and other.pending_flags() == [] and L.control(other) == want[3]
    rest, _ = L.run_steps(other, xt, y, 3, first=4)
    scale, skipped, good, _c = want[3]
    assert good + 1 == L.INTERVAL
    # nothing to apply until its own first flag is 2 steps old; that one is the third clean flag in a row
    assert rest == [want[3], want[3], (2 * scale, skipped, 0, 0)]


def test_divergence_shows_at_one_step_index(cuda, setup, spin):
    """max_consecutive_skips = 3 and an Inf in every step: diverged(), asked after every step as fit() asks, first says yes
    after the same step on the eager and on the lazy twin -- the step the reference names."""
    params, xt, anns = setup
    cycles, _ms, _rate = spin
    steps = 7
    want = R.loss_scale_ref([1] * steps, L.LAG, SCALE0, L.INTERVAL)
    first = next(i for i in range(steps) if want[i][3] >= 3)
    assert first == 4  # the flags of steps 0, 1, 2 are applied at steps 2, 3, 4
    firsts = {}
    for name, kw in (("eager", dict(eager=True)), ("lazy", dict(spin=cycles))):
        tr = _trainer(cuda, params)
        tr.max_consecutive_skips = 3
        said = []
        hist, flags = L.run_steps(tr, xt, _target(tr, anns), steps, inject=range(steps), after_step=lambda i: said.append(tr.diverged()),
                                  **kw)
        assert flags.cpu().tolist() == [1] * steps
        assert hist == want, name
        firsts[name] = said.index(True)
        assert said == [i >= firsts[name] for i in range(steps)]
    assert firsts == {"eager": first, "lazy": first}
