"""Regenerates tests/golden/cubed_sphere_case.json from the reference (GHEX v0.8.0). Run by hand
where the reference tree is available; never by a test:

    python tests/golden/make_cubed_sphere_case.py --reference <GHEX tree> --workdir <scratch dir>

Compiles tests/golden/cubed_sphere_driver.cpp against the reference's header-only halo generator
(g++ -std=c++17; an empty ghex/config.hpp is put into the work directory), feeds it the
configurations below and stores its output: per configuration and domain every generated halo
box (local, global, tile), the neighbour-tile images of the local cells first, first + (1, 0)
and first + (0, 1), the two vector sign factors evaluated from transform_lu as
cubed_sphere/field_descriptor.hpp:98-104 does, and the non-empty seven-argument intersections
with every domain. Record layout: see tests/cs_cases.py."""
import argparse
import json
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def configurations():
    """(edge_size, levels, halos (-x, +x, -y, +y), domains [(tile, xf, xl, yf, yl)])."""
    ref = [(t, xf, xf + 4, yf, yf + 4) for t in range(6) for (xf, yf) in
           ((0, 0), (5, 0), (0, 5), (5, 5))]  # test_cubed_sphere_exchange.cpp:945-955
    return [
        (10, 3, (2, 2, 2, 2), ref),
        (6, 2, (1, 2, 0, 3), [(t, 0, 5, 0, 5) for t in range(6)]),
        (70, 5, (3, 3, 3, 3), [(t, 0, 69, 0, 69) for t in range(6)]),
        (8, 2, (2, 2, 2, 2), [(t, xf, xf + 3, 0, 7) for t in range(6) for xf in (0, 4)]),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--workdir", required=True)
    a = ap.parse_args()
    os.makedirs(os.path.join(a.workdir, "inc", "ghex"), exist_ok=True)
    open(os.path.join(a.workdir, "inc", "ghex", "config.hpp"), "w").close()
    exe = os.path.join(a.workdir, "cubed_sphere_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(a.reference, "include"), "-I",
                    os.path.join(a.workdir, "inc"), os.path.join(HERE, "cubed_sphere_driver.cpp"),
                    "-o", exe], check=True)
    cfgs = configurations()
    text = [str(len(cfgs))]
    for c, levels, halos, doms in cfgs:
        text.append(" ".join(map(str, (c, levels, *halos, len(doms)))))
        text.extend(" ".join(map(str, d)) for d in doms)
    out = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True,
                         check=True).stdout
    data = json.loads(out)
    with open(os.path.join(HERE, "cubed_sphere_case.json"), "w") as fh:
        json.dump(data, fh, separators=(",", ":"))
        fh.write("\n")
    print(f"{len(data)} configurations, {sum(len(c['domains']) for c in data)} domains")


if __name__ == "__main__":
    main()
