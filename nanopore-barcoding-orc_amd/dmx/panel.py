"""Adapter panels: FASTA parsing and cutadapt-style adapter specifications.

Restates cutadapt 4.9's parser behaviour for the forms the reference uses
(scripts/02_cutadapt_loop.sh:69 `-g file:SP5.fa`, :99 `-a file:SP27rc.fa`;
scripts/04_cleaning_primers.sh:377 `-g FWD...REV`, :476-498 `-g SEQ` / `-a SEQ`):
  * `file:PATH`: one adapter per FASTA record; name = first word of the header line;
  * `NAME=SEQ` or `SEQ`: a literal adapter, auto-named "1", "2", ... in command-line order;
  * `A...B`: a linked adapter (front A, back B);
  * `-g ^SEQ` / `-a SEQ$`: anchored (PrefixAdapter / SuffixAdapter: the whole adapter at the read
    start / end, minimum overlap = its length whatever -O says); `-g XSEQ` / `-a SEQX`:
    non-internal (NonInternalFrontAdapter / NonInternalBackAdapter; any number of X is stripped).
    `^` or a leading X with -a, `$` or a trailing X with -g, `^` with a leading X and `$` with a
    trailing X are refused (SpecError), as parser.py refuses them; the markers are read per
    record of a `file:` panel;
  * sequences uppercased with U -> T (upstream parser.py; UNVERIFIED).
The panels in the reference have no trailing newline (M13_amplicon_indices_forward.fa:24) and
blank lines (RNA_primers.fa:5); both are tolerated.
"""
from __future__ import annotations

import os
import re
from dataclasses import dataclass, field

DATA_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")
SP5_FASTA = os.path.join(DATA_DIR, "M13_amplicon_indices_forward.fa")
SP27RC_FASTA = os.path.join(DATA_DIR, "M13_amplicon_indices_reverse_rc.fa")
COI_FASTA = os.path.join(DATA_DIR, "COI_primers.fa")
RNA_FASTA = os.path.join(DATA_DIR, "RNA_primers.fa")

IUPAC = set("ACGTURYSWKMBDHVN")


def normalize(seq: str) -> str:
    s = seq.strip().upper().replace("U", "T")
    bad = set(s) - IUPAC
    if bad:
        raise ValueError(f"adapter {seq!r} contains non-IUPAC characters {sorted(bad)}")
    if not s:
        raise ValueError("empty adapter sequence")
    return s


def read_fasta(path: str) -> list[tuple[str, str]]:
    """Parse a FASTA file into (header, sequence) records (whitespace inside sequences dropped)."""
    recs: list[tuple[str, str]] = []
    header, parts = None, []
    with open(path, "r") as fh:
        for line in fh:
            line = line.rstrip("\r\n")
            if not line.strip():
                continue
            if line.startswith(">"):
                if header is not None:
                    recs.append((header, "".join(parts)))
                header, parts = line[1:], []
            else:
                if header is None:
                    raise ValueError(f"{path}: sequence before the first '>' header")
                parts.append("".join(line.split()))
    if header is not None:
        recs.append((header, "".join(parts)))
    return recs


class SpecError(ValueError):
    """An adapter specification cutadapt refuses, or one outside the implemented subset: the
    command line exits with status 2 and this message."""


@dataclass
class Adapter:
    name: str
    seq: str
    where: str            # "front" (-g) or "back" (-a)
    restrict: str = ""    # "", "anchored" (^SEQ / SEQ$) or "noninternal" (XSEQ / SEQX)
    min_overlap: int | None = None   # None: the call's -O; anchored: the adapter's length

    @property
    def type_name(self) -> str:
        """The "type" of this adapter's end in the JSON report: cutadapt's anchored_five_prime,
        noninternal_five_prime, anchored_three_prime, noninternal_three_prime; an unrestricted
        adapter keeps the "regular" this report has always written."""
        end = "five_prime" if self.where == "front" else "three_prime"
        return f"{self.restrict}_{end}" if self.restrict else "regular"


def split_markers(spec: str, where: str) -> tuple[str, str]:
    """(sequence, restriction) of one single-adapter specification (parser.py
    _parse_not_linked / _restriction_to_class): restriction is "", "anchored" or
    "noninternal"."""
    s = spec.strip()
    front = back = ""
    if s.startswith("^"):
        front, s = "anchored", s[1:]
    if s.upper().startswith("X"):
        if front:
            raise SpecError(f"adapter {spec!r}: either '^' (anchored) or a leading 'X' "
                            "(non-internal), not both")
        front, s = "noninternal", s.lstrip("xX")
    if s.endswith("$"):
        back, s = "anchored", s[:-1]
    if s.upper().endswith("X"):
        if back:
            raise SpecError(f"adapter {spec!r}: either '$' (anchored) or a trailing 'X' "
                            "(non-internal), not both")
        back, s = "noninternal", s.rstrip("xX")
    if front and back:
        raise SpecError(f"adapter {spec!r}: restricted at both ends; use a linked adapter")
    if where == "front" and back:
        raise SpecError(f"adapter {spec!r}: '$' or a trailing 'X' belongs to a 3' adapter "
                        "(-a), not to -g")
    if where == "back" and front:
        raise SpecError(f"adapter {spec!r}: '^' or a leading 'X' belongs to a 5' adapter "
                        "(-g), not to -a")
    return s, front or back


@dataclass
class LinkedAdapter:
    name: str
    front: str
    back: str


@dataclass
class AdapterSet:
    adapters: list = field(default_factory=list)   # Adapter or LinkedAdapter, command-line order
    _counter: int = 0

    def _auto_name(self) -> str:
        self._counter += 1
        return str(self._counter)

    def add_spec(self, spec: str, where: str):
        """Add one -g/-a argument."""
        # `-g ^file:PATH` / `-a file:PATH$` anchor every record of the file (cutadapt's documented
        # demultiplexing form); records may also carry their own markers
        pre = "^" if spec.startswith("^file:") else ""
        if pre or spec.startswith("file:"):
            path = spec[len(pre) + 5:]
            post = ""
            if path.endswith("$") and not os.path.exists(path):
                path, post = path[:-1], "$"
            for header, seq in read_fasta(path):
                name = header.split()[0] if header.split() else self._auto_name()
                self._add(name, pre + seq.strip() + post, where)
            return
        name = None
        if "=" in spec:
            name, spec = spec.split("=", 1)
            name = name.strip()
        if "..." in spec:
            a, b = spec.split("...", 1)
            if any(ch and ch in "^$xX" for ch in (a[:1], a[-1:], b[:1], b[-1:])):
                raise SpecError(f"adapter {spec!r}: anchored / non-internal parts of a linked "
                                "adapter are out of scope (single adapters take ^, $ and X)")
            if where != "front":
                # -a A...B is also linked in cutadapt (front optional by default); not used by
                # the reference scripts.
                raise NotImplementedError("linked adapters are supported with -g only")
            self.adapters.append(LinkedAdapter(name or self._auto_name(), normalize(a),
                                               normalize(b)))
            return
        self._add(name or self._auto_name(), spec, where)

    def _add(self, name: str, seq: str, where: str):
        s, restrict = split_markers(seq, where)
        s = normalize(s)
        self.adapters.append(Adapter(name, s, where, restrict,
                                     len(s) if restrict == "anchored" else None))

    @property
    def linked(self) -> bool:
        return any(isinstance(a, LinkedAdapter) for a in self.adapters)


def load_panel(path: str) -> tuple[list[str], list[str]]:
    """(names, sequences) of a FASTA panel."""
    recs = read_fasta(path)
    return [h.split()[0] for h, _ in recs], [normalize(s) for _, s in recs]


_PAIR_ID = re.compile(r"_([A-Z])(?=\s|$|_)")


def primer_pairs(path: str) -> list[tuple[str, str, str]]:
    """Linked primer pairs [(pair_id, forward, reverse)] from a round-1 primer FASTA.

    Restates the header convention of scripts/04_cleaning_primers.sh:184-270: a header holding
    "Forward" / "Reverse" assigns its sequence to every pair id `_X` it carries (X one capital
    letter followed by whitespace, `_` or the end); pair order = first appearance; a later
    record for the same (id, orientation) replaces the earlier one; incomplete pairs are skipped
    (:380-385).  The sequences are used as written (the script does not reverse-complement)."""
    fwd: dict[str, str] = {}
    rev: dict[str, str] = {}
    order: list[str] = []
    for head, seq in read_fasta(path):
        seq = "".join(seq.split())
        if not seq:
            continue
        ids = _PAIR_ID.findall(">" + head)
        if "Forward" in head:
            dst = fwd
        elif "Reverse" in head:
            dst = rev
        else:
            continue
        for pid in ids:
            dst[pid] = seq
            if pid not in order:
                order.append(pid)
    return [(p, fwd[p], rev[p]) for p in order if p in fwd and p in rev]
