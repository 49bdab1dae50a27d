"""Shared by tests/test_gpu_loss_scale_schedule.py, tests/test_gpu_dp.py and tests/dp_schedule_worker.py: training steps run in
pieces with the loss-scale control's values recorded at the start of every step, an Inf injected into chosen steps, and a
spin kernel that keeps a step's flag copy in flight while the host starts the next steps.  Not a test module."""
import time

import torch

LAG = 2  # the contract: the flag of step j is applied at the start of step j + 2
INTERVAL = 3  # loss_scale_growth_interval of every run here: 8 steps see the scale double
INJECT = (2, 5)
FLAGS = [0, 0, 1, 0, 0, 1, 0, 0]  # the device flags of 8 steps with an Inf injected at INJECT
SPIN_STEPS = 4  # the lazy twin's spin, in durations of one step


def control(tr):
    return (tr.loss_scale, tr.skipped_steps, tr._good_steps, tr._consecutive_skips)


def ticks_per_ms():
    """The rate of the clock torch.cuda._sleep counts, measured (not assumed) as detector.stream_queue_sets measures it."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1000)  # first launch: module load
    e0.record()
    torch.cuda._sleep(200000)
    e1.record()
    e1.synchronize()
    return 200000 / max(e0.elapsed_time(e1), 1e-3)


def run_steps(tr, xt, y, steps, inject=(), spin=0, eager=False, after_step=None, first=0):
    """`steps` steps in the pieces of Trainer.step.  inject: step indices whose loss gradient gets an Inf, the way
    test_gpu_trainer_update.py injects it.  spin: cycles of torch.cuda._sleep queued between allreduce() and sgd(), so that the
    step's update and its flag copy are still in flight when the host begins the next step (the lazy twin).  eager: the host
    waits for the device after every step.  after_step(i) runs behind step i.
    -> (the control's values at the START of every step, the device flag of every step as a device tensor [steps])"""
    hist = []
    flags = torch.zeros(steps, dtype=torch.int32, device=tr.device)
    for i in range(first, first + steps):
        tr._poll_nonfinite()
        hist.append(control(tr))
        tr.forward(xt)
        tr.loss(y)
        if i in inject:
            tr.grad_pred[0, 5, 3] = float("inf")  # what an overflowing loss gradient looks like
        tr.backward()
        tr.allreduce()
        if spin:
            torch.cuda._sleep(int(spin))
        tr.sgd()
        flags[i - first].copy_(tr.nonfinite[0])
        if eager:
            torch.cuda.synchronize()
        if after_step is not None:
            after_step(i)
    return hist, flags


def measure_step_ms(tr, xt, y, warm=3, steps=5):
    """Milliseconds per step of `tr` on this batch, host and device together (at 2 x 96^2 the host's launches are the longer
    half); the trainer's control is drained afterwards and is NOT the fresh one."""
    run_steps(tr, xt, y, warm)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run_steps(tr, xt, y, steps)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    tr._poll_nonfinite(wait=True)
    return ms
