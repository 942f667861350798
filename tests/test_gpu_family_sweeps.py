"""Seeded random rows (tests/sweep_cases.py) through the kernels on an MI355X: one test per sweep and seed, 24 rows each, every
row run by the runner its family's instance module uses (tests/family_runners.py) and judged by the reference and bar of its
family's table - bit equality or the long-double bars, nothing new.  The launch record is compared with the family's mirror on
every row, through LaunchLogs of this module's own.  A row that fails its table's admission condition is skipped and counted; the
host module (tests/test_sweep_cases_host.py) keeps the skipped share at or below 10 %.  A failure names sweep, seed, index and the
row, so that sweep_cases.draw(sweep, seed, index) rebuilds it.  The last test checks that the sweeps together saw every kernel name
their families' instance tables enumerate."""
import time

import pytest

import sweep_cases as sw
from family_runners import JUDGES, LAUNCH_READERS
from gpu_harness import LaunchLog, torch_gpu  # noqa: F401  (torch_gpu: the fixture)
from gpu_harness import lib as _lib

pytestmark = pytest.mark.gpu

LOGS = {family: LaunchLog(reader, joined=joined) for family, (reader, joined) in LAUNCH_READERS.items()}
RAN = set()


@pytest.mark.parametrize("seed", sw.SEEDS)
@pytest.mark.parametrize("sweep", list(sw.SWEEPS))
def test_sweep(torch_gpu, sweep, seed):
    S = sw.SWEEPS[sweep]
    skipped, worst, t_ref, t_gpu = 0, 0.0, 0.0, 0.0
    for index in range(sw.ROWS_PER_SEED):
        t0 = time.perf_counter()
        row = sw.draw(sweep, seed, index)
        case = sw.case(sweep, row)
        t1 = time.perf_counter()
        t_ref += t1 - t0
        if not S.admitted(row, case):
            skipped += 1
            continue
        try:
            worst = max(worst, JUDGES[sweep](torch_gpu, row, case, LOGS[S.family]))
        except Exception as e:                               # whatever went wrong, say which row: draw(sweep, seed, index) rebuilds it
            raise AssertionError(f"sweep {sweep}, seed {seed}, index {index}: {type(e).__name__}: {e}\nrow: {row}") from e
        t_gpu += time.perf_counter() - t1
    print(f"{sweep} seed {seed}: {sw.ROWS_PER_SEED - skipped} rows run, {skipped} skipped, worst |err| / bar {worst:.3g}, "
          f"reference {t_ref:.2f} s, GPU calls and checks {t_gpu:.2f} s")
    assert skipped <= sw.MAX_SKIPPED * sw.ROWS_PER_SEED
    RAN.add((sweep, seed))


def test_the_sweeps_saw_every_instance(torch_gpu):
    assert RAN == {(s, seed) for s in sw.SWEEPS for seed in sw.SEEDS}, "run with the sweeps of this module"
    lib = _lib()
    for family, log in LOGS.items():
        count, name = getattr(lib, f"hsr_{family}_instance_count"), getattr(lib, f"hsr_{family}_instance_name")
        table = {name(i).decode() for i in range(count())}
        assert log.seen == table, (family, sorted(table - log.seen), sorted(log.seen - table))
        print(f"{family}: {len(log.seen)} of {len(table)} instances seen")
