"""CPU: the entry table of tests/test_streams_gpu.py against include/packppi_hip.h.

Every export that takes a ``void *stream`` is a row of the GPU table or is exempt with a reason; neither list names an export that is
gone.  A new stream-taking entry point then cannot be added without a test on a busy stream."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stream_taking_exports():
    """Names of the header's ``pp_status pp_*( ... void *stream ... )`` prototypes, the PP_DIAG block included."""
    src = open(os.path.join(ROOT, "include", "packppi_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = re.findall(r"\bpp_status\s+(pp_\w+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
    return sorted(name for name, args in protos if re.search(r"\bvoid\s*\*\s*stream\b", args))


def all_exports():
    src = open(os.path.join(ROOT, "include", "packppi_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(pp_[a-z0-9_]+)\s*\(", src))


def _lists():
    from . import test_streams_gpu as G          # imports torch, never touches the device
    return G.TABLE_ENTRIES, G.EXEMPT, G.ROWS


def test_the_header_parse_finds_the_entries():
    names = stream_taking_exports()
    assert len(names) >= 37 and {"pp_score", "pp_sample_corrected", "pp_polar", "pp_so2_score", "pp_debug_edge"} <= set(names)
    assert "pp_plan_create" not in names and "pp_profile_read" not in names and "pp_ctx_destroy" not in names


def test_every_stream_taking_export_has_a_row_or_a_reason():
    table, exempt, _ = _lists()
    missing = [n for n in stream_taking_exports() if n not in table and n not in exempt]
    assert not missing, f"stream-taking exports without a row in tests/test_streams_gpu.py ROWS and without an EXEMPT entry: {missing}"
    assert not set(table) & set(exempt), sorted(set(table) & set(exempt))
    assert all(isinstance(r, str) and len(r) > 20 and "\n" not in r for r in exempt.values())


def test_no_row_or_exemption_names_an_export_that_is_gone():
    table, exempt, rows = _lists()
    have, takes = all_exports(), set(stream_taking_exports())
    gone = [n for n in list(table) + list(exempt) if n not in have]
    assert not gone, f"tests/test_streams_gpu.py names exports the header no longer declares: {gone}"
    assert not [n for n in list(table) + list(exempt) if n not in takes], "a listed export takes no stream"
    ids = [r.id for r in rows]
    assert len(ids) == len(set(ids))


def test_the_rows_the_header_marks_as_not_waiting_assert_it():
    """Every export whose comment says it never waits for the stream has at least one row with never_waits."""
    src = open(os.path.join(ROOT, "include", "packppi_hip.h")).read()
    _, _, rows = _lists()
    asserted = {r.entry for r in rows if r.never_waits}
    marked = []
    for m in re.finditer(r"/\*(.*?)\*/\s*(?:#define[^\n]*\n\s*)*pp_status\s+(pp_\w+)\s*\(", src, flags=re.S):
        text = " ".join(m.group(1).split())
        if re.search(r"[Nn]ever waits for the stream|never waits for the stream|Does not wait for the stream", text):
            marked.append(m.group(2))
    assert len(marked) >= 8, marked
    assert not [n for n in marked if n not in asserted and n != "pp_ctx_set_obstacles"], (marked, sorted(asserted))
