#!/usr/bin/env python3
"""A/B on the box this is started on (boxes differ by up to 30 %, so only numbers of one call compare): a command run under several variants
in turn, `--rounds` times over.

A variant is a prebuilt library, copied over --target for its steps (--lib NAME=FILE, repeatable; tools/mkvariant.sh builds one), or an
environment, put in front of the command as `env` would (--env "A=1 B=2", repeatable; --env "" is the caller's environment as it is).  Within
a round every variant runs the command once per argument set (--args "--batch 256|--batch 4096": each set is appended to the command), so the
variants alternate: round 1: a, b; round 2: a, b.  --warmup COMMAND runs once first and is not reported.
Every step runs under `timeout -k 10 <--limit>`.  After the first step that ends with a status other than 0 - a fault, an abort, the time
limit - nothing more is started, and that status is the exit status.  Whatever happens, the target is put back from a copy kept beside it.
Per step one line: the variant, the argument set and, if the command's last line of stdout is a bench.py line, its value, ms_per_step, fused
value and kernel_ms_per_step; otherwise that last line as it is (a hash from tools/probes/sol_hash.py, the summary of a pytest run).
No environment variable is set here and none is changed.
usage (GPU box, repository root): python tools/ab.py --lib head=FILE --lib work=FILE [--args "--batch 256|--batch 4096"] [--rounds 2] [--limit 300]
       [--warmup COMMAND] [--target FILE] [-- COMMAND ...]        (default command: python bench.py --full --cpu-sample 0)
"""
import argparse
import json
import os
import shlex
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMAND = ["python", "bench.py", "--full", "--cpu-sample", "0"]


def run_step(env, command, limit):
    """(exit status, last line of stdout) of the command under its time limit, `env` (a list of NAME=VALUE) in front of it"""
    cmd = (["env"] + env if env else []) + ["timeout", "-k", "10", str(limit)] + command
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    return r.returncode, (r.stdout.strip().splitlines() or [""])[-1]


def report(text):
    """the four fields of a bench.py line, or the line as it is"""
    try:
        d = json.loads(text)
        return "%s %s %s %s" % (d["value"], d["ms_per_step"], (d.get("fused") or {}).get("value"), d["kernel_ms_per_step"])
    except (ValueError, KeyError, TypeError, AttributeError):
        return text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", default=[], metavar="NAME=FILE", help="a variant: FILE is copied over --target for its steps")
    ap.add_argument("--env", action="append", default=[], metavar='"A=1 B=2"', help="a variant: these settings in front of the command")
    ap.add_argument("--args", default="", help="argument sets appended to the command, separated by |")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--limit", type=int, default=300, help="time limit of one step [s]")
    ap.add_argument("--warmup", help="a command run once before the first round, not reported")
    ap.add_argument("--target", default=os.path.join(ROOT, "bipedal_control_amd", "libbpmpc.so"), help="the file a library variant is copied over")
    ap.add_argument("command", nargs="*", help="after --: the command (default: %s)" % " ".join(COMMAND))
    a = ap.parse_args()
    libs = [v.split("=", 1) for v in a.lib]
    for name, path in libs:
        if not os.path.isfile(path):
            ap.error("--lib %s: no file %s" % (name, path))
    variants = [(name, path, []) for name, path in libs] + [("[%s]" % e, None, shlex.split(e)) for e in a.env]
    if not variants:
        ap.error("no variant: give --lib or --env")
    command = a.command or COMMAND
    keep = a.target + ".ab_keep"
    if libs:
        shutil.copyfile(a.target, keep)
    status = 0
    try:
        if a.warmup:
            status, _ = run_step([], shlex.split(a.warmup), a.limit)
        steps = [(v, args) for _ in range(a.rounds) for v in variants for args in a.args.split("|")]
        for (name, path, env), args in steps:
            if status != 0:
                break
            if libs:
                shutil.copyfile(path or keep, a.target)
            status, text = run_step(env, command + shlex.split(args), a.limit)
            print("%s [%s] %s" % (name, args.strip(), report(text) if status == 0 else "ended with status %d" % status), flush=True)
        if status != 0:      # nothing more is started on the GPU
            print("ab: a step ended with status %d; stopping" % status, file=sys.stderr)
    finally:
        if libs:
            shutil.copyfile(keep, a.target)
            os.remove(keep)
    return status if status >= 0 else 1


if __name__ == "__main__":
    sys.exit(main())
