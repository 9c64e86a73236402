"""Every function of include/diffsg.h that takes a stream has a case in tests/test_gpu_streams.py (run on a non-default stream there), or
an exemption with its reason here.  Runs without a device: a new entry point cannot be added without a stream case."""
import os
import re

from _util import ROOT
import test_gpu_streams as G

# Not run under the deferred-input protocol, and why.
EXEMPT = {
    "dsg_range_status_stream": "a query whose purpose is to synchronise `stream`; reached through the DDPM.sample cases (py-sample-*), "
                               "which list it as their reason to synchronise",
    "dsg_time_op": "bench.py's measurement hook: times a replay with HIP events and waits for them; no caller input is read on the device",
    "dsg_box_calibrate": "bench.py's box probe: fixed internal kernels timed with HIP events it waits for; no caller input at all",
}


def stream_functions():
    """Names of the functions declared in the header whose parameter list ends in `void* stream`."""
    with open(os.path.join(ROOT, "include", "diffsg.h")) as f:
        src = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    decls = re.findall(r"\b(dsg_\w+)\s*\(([^()]*)\)\s*;", src)
    return sorted(name for name, params in decls if re.search(r"void\s*\*\s*stream\s*$", params.strip()))


def test_the_parser_sees_the_header():
    """Known members and non-members, so that a header reformatting that blinds the parser fails here and not silently."""
    names = stream_functions()
    assert len(names) >= 35, names
    for n in ("dsg_bind_weights", "dsg_sample_chunked", "dsg_train_step_seeded_dyn", "dsg_best_of", "dsg_gd_nu", "dsg_ppo_train_epoch",
              "dsg_box_calibrate"):
        assert n in names, n
    for n in ("dsg_create", "dsg_range_status", "dsg_set_option", "dsg_mlp_param_total", "dsg_train_profile"):
        assert n not in names, n


def test_every_stream_taking_function_has_a_stream_case_or_an_exemption():
    covered = {e for c in G.CASES for e in c.entries}
    names = stream_functions()
    missing = [n for n in names if n not in covered and n not in EXEMPT]
    assert not missing, f"no case in tests/test_gpu_streams.py (and no exemption) for: {missing}"
    assert not [n for n in EXEMPT if n not in names], "an exemption names a function the header does not declare with a stream"
    assert not [e for e in covered if e not in names], "a case names a function the header does not declare with a stream"
    assert all(reason.strip() for reason in EXEMPT.values())


def test_the_table_is_well_formed():
    ids = [c.id for c in G.CASES]
    assert len(set(ids)) == len(ids)
    for c in G.CASES:
        assert c.entries and callable(c.build), c.id
        assert c.sync is None or (isinstance(c.sync, str) and len(c.sync) > 20), c.id     # a synchronising case says why
