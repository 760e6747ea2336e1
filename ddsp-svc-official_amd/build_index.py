"""Builds the unit index file that `main.py --index` reads, from the `units/` tree `preprocess.py` wrote:

    python build_index.py -i data/train --spk 1 -o voice1.pt [--centres 10000] [--iters 10] [--max_entries N] [-d cuda]

Every stored unit of the speaker (all speakers without `--spk`) is read; `--max_entries` keeps an evenly strided subset first;
what is left is reduced to at most `--centres` k-means centres on the device (`infer_offline.UnitIndex.reduce`: a deterministic
rule of this project, stated in include/ddsp_amd.h at `ddsp_units_kmeans_assign`).  A tree with no more rows than `--centres`
is saved as it is.  One line is printed: entries in, centres out, empty centres dropped, and the entries that still changed
centre in the last iteration."""
import argparse
import sys

from controls import UnitIndex


def parse_args(args=None):
    parser = argparse.ArgumentParser(description="unit index of a voice for main.py --index, reduced to k-means centres")
    parser.add_argument("-i", "--input", type=str, required=True, help="the data path that holds units/ (preprocess.py's output)")
    parser.add_argument("-o", "--output", type=str, required=True, help="the index file to write")
    parser.add_argument("--spk", type=str, default=None, help="speaker folder under units/ (default: all folders)")
    parser.add_argument("--centres", type=int, default=10000, help="k-means centres to reduce to (default 10000)")
    parser.add_argument("--iters", type=int, default=10, help="full Lloyd iterations (default 10; 0: the strided subset)")
    parser.add_argument("--max_entries", type=int, default=None, help="keep an evenly strided subset of this many rows first")
    parser.add_argument("-d", "--device", type=str, default="cuda", help="the HIP device of the reduction")
    cmd = parser.parse_args(args)
    for name, low in (("centres", 1), ("iters", 0), ("max_entries", 1)):
        v = getattr(cmd, name)
        if v is not None and v < low:
            parser.error(f"--{name} must be an int >= {low}, got {v}")
    return cmd


def build(cmd):
    """-> (the index written to cmd.output, entries in, the reduction's report)."""
    full = UnitIndex.from_units_dir(cmd.input, spk=cmd.spk, max_entries=cmd.max_entries)
    index, report = full.reduce(cmd.centres, iters=cmd.iters, device=cmd.device, report=True)
    index.save(cmd.output)
    return index, len(full), report


def main(args=None):
    cmd = parse_args(args)
    index, entries, report = build(cmd)
    last = report["moved"][-1] if report["moved"] else 0
    print(f"{cmd.output}: {entries} entries in, {len(index)} centres out, {report['dropped']} dropped, moved in the last "
          f"iteration {last}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
