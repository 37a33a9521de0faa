"""Records which names of the reference's public headers the reference-side adapter (integration/hip_batch_solver.cpp) relies on, into
tests/golden/ref_adapter_surface.json, so that tests/test_integration_adapter.py checks them without a reference checkout.
Names only: the header paths under include/cddp-cpp/{cddp_core,dynamics_model}/ and, per header the test reads, the identifiers, zero-argument
calls `name()`, `class` / `struct` names and `using` aliases it contains -- restricted to names the adapter or the test mention.
Run where a cddp-cpp checkout is present:   python tests/golden/make_ref_adapter_surface.py <cddp-cpp checkout>"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "ref_adapter_surface.json")
FILES = ("cddp_core/cddp_core.hpp", "cddp_core/constraint.hpp", "cddp_core/terminal_constraint.hpp", "cddp_core/objective.hpp",
         "cddp_core/dynamical_system.hpp", "cddp_core/options.hpp", "cddp_core/boxqp.hpp", "dynamics_model/pendulum.hpp",
         "dynamics_model/cartpole.hpp", "dynamics_model/lti_system.hpp")
IDENT = r"[A-Za-z_][A-Za-z0-9_]*"


def main(ref_root):
    inc = os.path.join(ref_root, "include", "cddp-cpp")
    if not os.path.isdir(inc):
        raise SystemExit("%s: no include/cddp-cpp" % ref_root)
    mentioned = set()
    for f in (os.path.join(REPO, "integration", "hip_batch_solver.cpp"), os.path.join(REPO, "tests", "test_integration_adapter.py")):
        mentioned |= set(re.findall(IDENT, open(f).read()))
    headers = sorted("%s/%s" % (d, f) for d in ("cddp_core", "dynamics_model")
                     for f in os.listdir(os.path.join(inc, d)) if f.endswith(".hpp"))
    files = {}
    for f in FILES:
        text = open(os.path.join(inc, f)).read()
        files[f] = {"identifiers": sorted(set(re.findall(r"\b%s\b" % IDENT, text)) & mentioned),
                    "nullary": sorted(set(re.findall(r"\b(%s)\(\)" % IDENT, text)) & mentioned),
                    "classes": sorted(set(re.findall(r"\b(?:class|struct)\s+(%s)" % IDENT, text)) & mentioned),
                    "aliases": sorted(set(re.findall(r"\busing\s+(%s)\s*=" % IDENT, text)) & mentioned)}
    json.dump({"source": "include/cddp-cpp of astomodynamics/cddp-cpp (names only)", "headers": headers, "files": files},
              open(OUT, "w"), indent=0, sort_keys=True)
    print("wrote", OUT)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
