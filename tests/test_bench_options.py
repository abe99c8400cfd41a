"""bench.py's command line: a plain ``--gpus 1 --steps N --warmup W`` run measures the headline only; ``--full``
(off by default) adds the part probes, the tuning check and the line's extras of the run as it was before."""
import inspect

import bench


def test_full_is_off_by_default():
    ap = bench.arg_parser()
    assert ap.parse_args(['--gpus', '1', '--steps', '5', '--warmup', '2']).full is False
    assert ap.parse_args(['--gpus', '1', '--steps', '5', '--warmup', '2', '--full']).full is True


def test_plain_run_measures_nothing_beside_the_headline():
    """source check (bench.run needs a GPU): every untimed measurement of the N* run sits behind --full"""
    head, tail = inspect.getsource(bench.run).split('if rank == 0:', 1)
    assert 'if args.full and not args.channels_last' in head          # store / clock probes, SMI readings
    assert 'if args.full and tuned is not None' in head               # the tuning check
    assert 'line_extras(args, w, elem, explicit, lib.dfm_plane_sweep_last_kernel()) if args.full else []' in tail


def test_full_run_keeps_its_extras():
    a = bench.arg_parser().parse_args(['--full'])
    assert bench.line_extras(a, bench.WORKLOADS['nstar'], 2, {}, 2) == \
        ['api_build_dfm_cost', 'channels_last_variant', 'traffic', 'secondary', 'cpu_baseline']
    a = bench.arg_parser().parse_args(['--full', '--no-secondary', '--no-cpu-baseline'])
    assert bench.line_extras(a, bench.WORKLOADS['nstar'], 2, {}, 2) == \
        ['api_build_dfm_cost', 'channels_last_variant', 'traffic']
