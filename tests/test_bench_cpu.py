"""bench.py's command line: a plain run times the steps and nothing else; --full adds the legs behind them."""
import bench

LEGS = ("no_cpu", "no_roofline", "no_live_pmc", "no_io", "no_extra", "no_sustained")


def test_plain_run_has_no_side_legs():
    a = bench.parse_args(["--steps", "3", "--warmup", "1"])
    assert not a.full and all(getattr(a, k) for k in LEGS)
    # asking to drop a leg of a plain run changes nothing
    assert vars(bench.parse_args(["--steps", "3", "--warmup", "1", "--no-cpu"])) == vars(a)


def test_full_runs_every_leg_unless_dropped():
    a = bench.parse_args(["--full"])
    assert a.full and not any(getattr(a, k) for k in LEGS)
    a = bench.parse_args(["--full", "--no-cpu", "--no-io"])
    assert a.no_cpu and a.no_io and not (a.no_roofline or a.no_live_pmc or a.no_extra or a.no_sustained)
