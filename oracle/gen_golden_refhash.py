#!/usr/bin/env python3
"""SHA-256 of what the reference's own C (oracle/_ref, oracle/build_ref.py) returns for the inputs of the two tests that
compare the oracle with it directly, so that those tests also hold where oracle/_ref cannot be built.

TEST INFRASTRUCTURE ONLY.  Run where the reference lies:

    python oracle/build_ref.py && python oracle/gen_golden_refhash.py

Writes tests/golden/refc_hashes.json (data only):
  entry_points/{cfg1,shipped}/<key>   every entry point the oracle and the compiled reference share, on the seeded block of
                                      tests/test_oracle_golden.py::shared_entry_points (images, loader tables, MISO
                                      outputs and the single-signal helpers)
  miso_small_table/cfg5/<key>         tests/test_oracle_golden.py::miso_small_table: MISO outputs and helpers at N = 1024
                                      on a five-direction seeded table
  receiver_shipped                    the frame the reference's receive_to_buffer builds from the seeded datagrams of
                                      tests/test_ingest.py, fed over a UDP loopback socket (n_arrays = 3)
Each recorded value is checked against the oracle before the file is written.
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (HERE, os.path.join(REPO, "zybo-rt-sampler-image-detection_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)
import das_oracle  # noqa: E402
import test_ingest  # noqa: E402
import test_oracle_golden  # noqa: E402
from configs import CONFIGS  # noqa: E402
from util import sha  # noqa: E402


def main():
    subprocess.check_call(["make", "-s", "-C", HERE, "libdas_oracle.so"])
    out = {"entry_points": {}}
    for name in ("cfg1", "shipped"):
        c = CONFIGS[name]
        ref = test_oracle_golden.shared_entry_points(das_oracle.RefLib(name), name)
        orc = test_oracle_golden.shared_entry_points(das_oracle.Oracle(c["N"], c["X"], c["Y"], c["T"]), name)
        for key in ref:
            assert ref[key].dtype == orc[key].dtype and ref[key].tobytes() == orc[key].tobytes(), (name, key)
        out["entry_points"][name] = {key: sha(a) for key, a in sorted(ref.items())}
        print(name, "%d entry points recorded" % len(ref), flush=True)
    out["miso_small_table"] = {}
    for name in ("cfg5",):
        c = CONFIGS[name]
        ref = test_oracle_golden.miso_small_table(das_oracle.RefLib(name), name)
        orc = test_oracle_golden.miso_small_table(das_oracle.Oracle(c["N"], c["X"], c["Y"], c["T"]), name)
        for key in ref:
            assert ref[key].dtype == orc[key].dtype and ref[key].tobytes() == orc[key].tobytes(), (name, key)
        out["miso_small_table"][name] = {key: sha(a) for key, a in sorted(ref.items())}
        print(name, "%d MISO / helper outputs on a small table recorded" % len(ref), flush=True)

    seed, n_arrays = 42, 3
    pk = test_ingest.datagrams(seed)
    got = test_ingest.receive_over_udp(C.CDLL(os.path.join(HERE, "_ref", "libref_receiver_shipped.so")), pk, n_arrays)
    assert got is not None, "cannot bind the replay socket"
    assert got.tobytes() == test_ingest.oracle_frame(None, pk, n_arrays).tobytes()
    out["receiver_shipped"] = {"seed": seed, "n_arrays": n_arrays, "packets_sha256": hashlib.sha256(pk.tobytes()).hexdigest(),
                               "frame_sha256": hashlib.sha256(got.tobytes()).hexdigest()}
    path = os.path.join(REPO, "tests", "golden", "refc_hashes.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)
    return 0


if __name__ == "__main__":
    sys.exit(main())
