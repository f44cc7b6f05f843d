"""Fold a file of sequences of mixed lengths through a few capacity contexts (ccj_amd.fold_many).

    python -m ccj_amd.batch [-d N] [-P set] [--noGU] [--contexts K] [--lockstep K] [--constraints] FILE

FILE holds one sequence per line, or FASTA records (a '>' header line, then the sequence over one
or more lines); '-' reads standard input.  Sequences are upper-cased and T becomes U, as the CCJ
command line does (ccj_amd/cli.py).  For every sequence, in input order, stdout gets exactly what
one CCJ run prints for it (cli.fold_cli: side messages, the sequence, "STRUCT (E)"; only the side
messages where the reference's backtrack exits) and stderr its stderr text; a sequence with a
character outside GCAU gets the command line's message and counts as exit code 1.  The exit code is
the largest one seen.  -P names a bundled parameter set or a .ccjp / .par path (default
DirksPierce09).  --lockstep K folds runs of K sequences of neighbouring length as one lockstep batch
(fold_many(lockstep=K)); the output is the same bytes.  Device: $CCJ_DEVICE, else $LOCAL_RANK, else 0.
--constraints: a sequence may be followed by one line over '.' and 'x' of its length (in a FASTA record:
after the sequence's last line); 'x' keeps that position unpaired (ccj_amd.Constraint).  A constraint
line of another length, or one that follows no sequence, gets a message on stderr, its sequence is not
folded and counts as exit code 1.  Without the flag the input grammar is unchanged.
"""
from __future__ import annotations

import argparse
import os
import sys

from . import fold_many, load_params
from .cli import fmt_energy


def read_sequences(lines) -> list:
    """One sequence per line, or FASTA; blank lines separate nothing and are skipped."""
    seqs, cur, fasta = [], None, False
    for raw in lines:
        line = raw.strip()
        if not line:
            continue
        if line.startswith(">"):
            fasta = True
            if cur:
                seqs.append(cur)
            cur = ""
        elif fasta:
            cur = (cur or "") + line
        else:
            seqs.append(line)
    if cur:
        seqs.append(cur)
    return [s.upper().replace("T", "U") for s in seqs]


def is_constraint_line(line: str) -> bool:
    return bool(line) and all(c in ".x" for c in line)


def read_records(lines) -> list:
    """The --constraints grammar: read_sequences' input in which a line over '.' and 'x' belongs to the
    sequence before it.  Returns (sequence, constraint line or None) pairs; a constraint line that
    follows no sequence, or a second one, is returned as ("", line)."""
    recs, cur, fasta = [], None, False   # cur: the open FASTA record [sequence, constraint]

    def attach(line):
        if recs and recs[-1][0] and recs[-1][1] is None:
            recs[-1][1] = line
        else:
            recs.append(["", line])

    for raw in lines:
        line = raw.strip()
        if not line:
            continue
        if line.startswith(">"):
            fasta = True
            if cur and cur[0]:
                recs.append(cur)
            cur = ["", None]
        elif is_constraint_line(line):
            if fasta and cur is not None and cur[0] and cur[1] is None:
                cur[1] = line
            elif fasta and cur is not None:
                if cur[0]:
                    recs.append(cur)
                    cur = ["", None]
                recs.append(["", line])
            else:
                attach(line)
        elif fasta:
            cur[0] += line
        else:
            recs.append([line, None])
    if cur and cur[0]:
        recs.append(cur)
    return [(s.upper().replace("T", "U"), c) for s, c in recs]


def record_stdout(rec) -> str:
    """What cli.fold_cli returns as stdout for one fold_many record."""
    seq, structure, energy, msgs, code, _ = rec
    if structure is None:
        return msgs
    return msgs + seq + "\n" + f"{structure} ({fmt_energy(energy)})\n"


def run(argv=None, stdout=None, stderr=None) -> int:
    stdout = stdout or sys.stdout
    stderr = stderr or sys.stderr
    ap = argparse.ArgumentParser(prog="python -m ccj_amd.batch", description=__doc__.splitlines()[0])
    ap.add_argument("-d", "--dangles", type=int, default=2)
    ap.add_argument("-P", "--paramFile", default="DirksPierce09")
    ap.add_argument("--noGU", action="store_true")
    ap.add_argument("--contexts", type=int, default=2)
    ap.add_argument("--lockstep", type=int, default=0)
    ap.add_argument("--constraints", action="store_true")
    ap.add_argument("file")
    a = ap.parse_args(argv)
    reader = read_records if a.constraints else read_sequences
    if a.file == "-":
        seqs = reader(sys.stdin)
    else:
        with open(a.file) as f:
            seqs = reader(f)
    cons = [None] * len(seqs)
    bad = {}
    if a.constraints:
        seqs, cons = [s for s, _ in seqs], [c for _, c in seqs]
        for x, (s, c) in enumerate(zip(seqs, cons)):
            if c is not None and len(c) != len(s):
                stderr.write(f"Constraint line of length {len(c)} for a sequence of length {len(s)}.\n")
                bad[x] = ""
    for x, s in enumerate(seqs):
        c = next((c for c in s if c not in "GCAU"), None)
        if c is not None and x not in bad:
            bad[x] = f"Sequence contains character {c} that is not G,C,A,U, or T.\n"
    good = [s for x, s in enumerate(seqs) if x not in bad]
    good_cons = [c for x, c in enumerate(cons) if x not in bad] if any(c is not None for c in cons) else None
    device = int(os.environ.get("CCJ_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    recs = iter(fold_many(good, a.dangles, params=load_params(a.paramFile), noGU=a.noGU, device=device,
                          contexts=a.contexts, lockstep=a.lockstep, constraints=good_cons))
    code = 0
    for x in range(len(seqs)):
        if x in bad:
            stdout.write(bad[x])
            code = max(code, 1)
            continue
        rec = next(recs)
        stdout.write(record_stdout(rec))
        stderr.write(rec[5])
        code = max(code, rec[4])
    stdout.flush()
    return code


if __name__ == "__main__":
    sys.exit(run())
