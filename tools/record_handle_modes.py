#!/usr/bin/env python3
"""Record what liodom_create decides for every handle of tests/handle_matrix.py on this device: per handle the config, the
switches set, the device's CU count and the full liodom_get_modes string right after creation (no scan processed).

    python tools/record_handle_modes.py [-o tests/handle_modes_mi355x.json]

The recording counts only if the concurrency probe passed (streams_concurrent=1) on every handle that asks for flags; the tool
exits with status 2 otherwise (the GPU was busy: record again)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import handle_matrix as hm      # noqa: E402
import liodom_amd as la         # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--out", default=os.path.join(ROOT, "tests", "handle_modes_mi355x.json"))
    a = ap.parse_args()
    for k in [k for k in os.environ if k.startswith("LIODOM_")]:
        del os.environ[k]
    entries, busy = [], []
    for entry in hm.MATRIX:
        group, name, p, c, sw = entry
        os.environ.update(sw)
        try:
            g = hm.create(la, entry)
        finally:
            for k in sw:
                del os.environ[k]
        modes = hm.modes_string(g)
        dev, cus = g.device_info()
        g.close()
        if "streams_concurrent=1" not in modes.split():
            busy.append(name)
        entries.append(dict(group=group, name=name, params=p, config=c, switches=sw, device=dev, cus=cus, modes=modes))
        print("%-28s %s" % (name, modes), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(entries, f, indent=1)
        f.write("\n")
    if busy:
        print("streams_concurrent=0 on: %s (the GPU was busy; record again)" % ", ".join(busy))
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
