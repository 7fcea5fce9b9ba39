"""The C ABI's statuses and messages that need no device, against the record (tests/golden/api_messages.json,
section "host", written by tools/record_api_messages.py): what a caller sees when an argument is wrong is part of
the interface, and csrc/rtg_api.cpp may be reorganised only with every one of them unchanged."""
import json
import os

import api_message_cases as cases
from conftest import GOLDEN


def _record(section):
    with open(os.path.join(GOLDEN, "api_messages.json")) as f:
        return json.load(f)[section]


def test_host_messages_match_the_record():
    """Every host case returns the recorded status and leaves the recorded text in rtg_last_error(), byte for byte;
    the ``nodev:`` cases -- valid calls that fail at their first device call -- run only where rtg_device_count() is
    0 and are compared up to and including the first ": " (the label is ours, the rest the HIP runtime's).

    The fail( sites of csrc/rtg_api.cpp that neither this section nor the "gpu" one (tests/test_gpu_api_messages.py)
    reaches, and why:
      - "host allocation failed" of the six constructors: a failed `new` of a small struct cannot be arranged;
      - hip_check behind every device call but a constructor's first (the later hipMalloc / hipMemcpy labels, the
        launch labels): they need a device that fails part-way; the first label of each constructor is pinned by its
        ``nodev:`` case, as are rtg_box_probe's, rtg_side_kernel_residency's and rtg_server_inbox_alloc's;
      - rtg_frame_server_post's "not served within": it needs a running server that stalls; no case launches;
      - take_device_error's "a previous launch reported device error": it needs a launch that sets the word
        (tests/test_gpu_edge.py::test_handover_timeout_is_reported_not_silent does that with a measurement build);
      - rtg_server_inbox_alloc's "not a large-BAR device": it needs a device without a large BAR; an MI355X has one
        and without a device the allocation before it fails."""
    from rtg import _lib
    lib = _lib.lib()
    want = _record("host")
    no_device = lib.rtg_device_count() == 0
    got = cases.run(cases.host_cases(lib), lib, no_device)
    expected = {k: v for k, v in want.items() if no_device or not k.startswith(cases.NODEV)}
    assert sorted(got) == sorted(expected), set(got) ^ set(expected)
    wrong = {k: (got[k], want[k]) for k in got if cases.comparable(k, got[k]) != cases.comparable(k, want[k])}
    assert not wrong, wrong


def test_record_is_complete_and_names_its_functions():
    """The record holds both sections, the device-failure cases carry a label, and every rejection that names a
    function names the one that was called (or, for rtg_local_rotation_multi_f32, the one it forwards to)."""
    host, gpu = _record("host"), _record("gpu")
    assert len(host) > 300 and len(gpu) > 100
    for k, (rc, msg) in host.items():
        if k.startswith(cases.NODEV):
            assert rc == 2 and ": " in msg, (k, rc, msg)   # RTG_ERR_DEVICE
    for sec in (host, gpu):
        for k, (rc, msg) in sec.items():
            assert (rc == 0) == (msg == ""), (k, rc, msg)
            if msg.startswith("rtg_"):
                group = k[len(cases.NODEV):] if k.startswith(cases.NODEV) else k
                group = group.split("/")[0].replace("local_rotation_multi", "kinematics_multi")
                assert msg.startswith("rtg_" + group), (k, msg)
