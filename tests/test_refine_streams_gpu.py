"""GPU: pp_chi_refine on a busy non-default stream (DESIGN.md sections 28 and 32).

The entry gets the rows every other geometry entry has in tests/test_streams_gpu.py, built with that file's own row builders and run
through the same gate (tests/stream_gate.py): the angles sit behind a device-side delay, the call is made without any
synchronisation, the outputs must equal the default-stream result bit for bit and the gate must still be pending when the call
returns (the header says that the entry never waits for the stream).  Two rounds of two sweeps: the second round reads the angles
the first one left on the device.

As tests/test_hnet_streams_gpu.py does, the rows are added on import to the lists that tests/test_streams_host.py holds against
include/packppi_hip.h: a run that collects this file sees the export covered; ``pytest tests/test_streams_host.py`` on its own
does not import this file and reports it as missing a row.
"""
import pytest

from . import stream_gate as SG
from . import test_streams_gpu as G
from .test_streams_gpu import world          # noqa: F401  (the module-scoped fixture: plan, batches and angles of the shapes)

pytestmark = pytest.mark.gpu


def _refine(c, x):
    res = c.refine_allatom(x, deltas_deg=(16, 8), max_sweeps=2, want_candidates=True)
    return {k: v for k, v in res.items() if k not in ("deltas", "fixed")}


ROWS = [G.Row("pp_chi_refine", case, G.chi_row(_refine), never_waits=True) for case in G.SHAPES]

# new lists, not appends: that file's own parametrised test keeps the table it was decorated with
G.ROWS = G.ROWS + [r for r in ROWS if r.id not in {q.id for q in G.ROWS}]
G.TABLE_ENTRIES = sorted({r.entry for r in G.ROWS})


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_entry_on_a_busy_stream(row, world):     # noqa: F811
    spec = row.make(world, row.case)
    SG.gated_call(spec["fn"], spec["inputs"], spec["poison"], entry=row.id, never_waits=row.never_waits)
    assert spec["ctx"].saturated() == 0
