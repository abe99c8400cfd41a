"""The one place that runs work on a second HIP stream.  ``fork_join(main_work, side_work, device)`` runs two independent
units of work, one on the caller's stream and one on the device's side stream, and joins them; it is also the one place
that applies rule 3 of derived.py: a step that built derived state makes the other stream wait for it.
Scratch is per (device, stream) (_launch.Workspace), so the two units share nothing but their inputs and those caches."""
import inspect

import torch

from .derived import derived_builds

_side_streams = {}   # device -> the side stream every fork on that device uses


def may_fork(device):
    return device.type == 'cuda' and not torch.cuda.is_current_stream_capturing()


def drain(steps):
    """run a generator of steps to its end -> its return value"""
    while True:
        try:
            next(steps)
        except StopIteration as done:
            return done.value


def _steps(work):
    if inspect.isgenerator(work):
        return work

    def one_step():
        return work()
        yield
    return one_step()


def _tensors(value):
    if torch.is_tensor(value):
        yield value
    elif isinstance(value, (tuple, list)):
        for v in value:
            yield from _tensors(v)


def fork_join(main_work, side_work, device, fork=True, alternate=False):
    """-> (main's result, side's result).  A unit of work is a callable or a generator that yields between steps and
    returns its result.  Steps are issued side first: the whole side unit, then main's, or -- ``alternate`` -- one step
    of each in turn, which keeps both streams fed when enqueueing a unit costs the host as long as running it.
    ``fork`` carries the caller's own conditions; where it is off, on a CPU device or during a capture the two units run
    main first on the current stream.  Both units stay referenced from here (and their inputs from the caller's frame)
    until after the join: the side stream reads tensors that were allocated on main."""
    main_steps, side_steps = _steps(main_work), _steps(side_work)
    if not (fork and may_fork(device)):
        return drain(main_steps), drain(side_steps)
    main = torch.cuda.current_stream(device)
    side = _side_streams.get(device)
    if side is None:
        side = _side_streams[device] = torch.cuda.Stream(device=device)
    todo, done, current = [(side, side_steps), (main, main_steps)], {}, main
    side.wait_stream(main)
    try:
        while todo:
            for turn in todo[:len(todo) if alternate else 1]:
                stream, steps = turn
                if stream is not current:   # (not once per step where a unit runs to its end)
                    torch.cuda.set_stream(stream)
                    current = stream
                built = derived_builds()
                try:
                    next(steps)
                except StopIteration as end:
                    done[steps] = end.value
                    todo.remove(turn)
                if derived_builds() != built:
                    # the step filled a cache with kernels on ITS stream; the other unit finds the cache filled and
                    # would read it unordered (in steady state nothing is built and the two streams run free)
                    for other, _ in todo:
                        if other is not stream:
                            other.wait_stream(stream)
    finally:
        torch.cuda.set_stream(main)
    main.wait_stream(side)
    for t in _tensors(done[side_steps]):
        t.record_stream(main)
    return done[main_steps], done[side_steps]
