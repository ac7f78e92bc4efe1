"""GPU: pp_hydrogens and pp_clashscore on a busy non-default stream (DESIGN.md sections 28 and 29).

The two entries get the rows every other geometry entry has in tests/test_streams_gpu.py, built with that file's own row builders and
run through the same gate (tests/stream_gate.py): the angles sit behind a device-side delay, the call is made without any
synchronisation, the outputs must equal the default-stream result bit for bit and the gate must still be pending when the call
returns (the header says that neither entry waits for the stream).

The rows live here, not in that file's table.  On import that module's ``ROWS`` and ``TABLE_ENTRIES`` are replaced by lists that
hold them too; tests/test_streams_host.py holds those lists against include/packppi_hip.h.  A run that collects this file (any run
of the whole suite, with or without a GPU) therefore sees the two exports covered; ``pytest tests/test_streams_host.py`` on its
own does not import this file and reports them as missing a row.
"""
import pytest

from . import stream_gate as SG
from . import test_streams_gpu as G
from .test_streams_gpu import world          # noqa: F401  (the module-scoped fixture: plan, batches and angles of the shapes)

pytestmark = pytest.mark.gpu

ROWS = [G.Row(entry, case, G.chi_row(call), never_waits=True)
        for entry, call in (("pp_hydrogens", lambda c, x: dict(c.hydrogens(chi=x))), ("pp_clashscore", lambda c, x: dict(c.clashscore(chi=x))))
        for case in G.SHAPES]

# new lists, not appends: that file's own parametrised test keeps the table it was decorated with
G.ROWS = G.ROWS + [r for r in ROWS if r.id not in {q.id for q in G.ROWS}]
G.TABLE_ENTRIES = sorted({r.entry for r in G.ROWS})


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_entry_on_a_busy_stream(row, world):     # noqa: F811
    spec = row.make(world, row.case)
    SG.gated_call(spec["fn"], spec["inputs"], spec["poison"], entry=row.id, never_waits=row.never_waits)
    assert spec["ctx"].saturated() == 0
