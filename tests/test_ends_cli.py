"""Anchored and non-internal adapters on the command line: parsing, refusals and report strings
without a GPU; one end-to-end drop-in run on the GPU, its files compared record for record with
records rendered from the demux oracle of ends_cases.py."""
import json
import subprocess

import numpy as np
import pytest

import ends_cases as ec
from dmx import cli, lib, panel
from dmx.report import Stats
from helpers import CLI, random_quals, read_fastq, write_fastq


def _parse(*specs):
    aset = panel.AdapterSet()
    for where, spec in specs:
        aset.add_spec(spec, where)
    return aset.adapters


def test_markers_parse_into_restricted_adapters(tmp_path):
    ads = _parse(("front", "^ACGTAC"), ("back", "bc2=TTGACA$"), ("front", "XXXGGATCC"),
                 ("back", "AAGCTTxx"), ("front", "plain=ACGGT"), ("back", "TTTGG"))
    assert [(a.seq, a.where, a.restrict, a.min_overlap) for a in ads] == [
        ("ACGTAC", "front", "anchored", 6), ("TTGACA", "back", "anchored", 6),
        ("GGATCC", "front", "noninternal", None), ("AAGCTT", "back", "noninternal", None),
        ("ACGGT", "front", "", None), ("TTTGG", "back", "", None)]
    assert [a.name for a in ads] == ["1", "bc2", "2", "3", "plain", "4"]
    assert lib.adapter_wheres(ads) == [ec.PREFIX, ec.SUFFIX, ec.FRONTX, ec.BACKX, ec.F, ec.B]
    assert [a.type_name for a in ads[:4]] == ["anchored_five_prime", "anchored_three_prime",
                                              "noninternal_five_prime",
                                              "noninternal_three_prime"]
    # file: panels take the markers per record; ^file: anchors every record
    fa = tmp_path / "p.fa"
    fa.write_text(">a first\n^ACGTACGT\n>b\nXTTGGCCAA\n>c\nGGGTTTAA\n")
    ads = _parse(("front", f"file:{fa}"))
    assert [(a.name, a.seq, a.restrict) for a in ads] == [
        ("a", "ACGTACGT", "anchored"), ("b", "TTGGCCAA", "noninternal"), ("c", "GGGTTTAA", "")]
    fb = tmp_path / "q.fa"
    fb.write_text(">a\nACGTACGT\n>b\nTTGGCCAA\n")
    assert [a.restrict for a in _parse(("front", f"^file:{fb}"))] == ["anchored"] * 2
    ads = _parse(("back", f"file:{fb}$"))
    assert [(a.restrict, a.where, a.min_overlap) for a in ads] == [("anchored", "back", 8)] * 2


REFUSED = [(["-a", "^ACGTACGT"], "^ACGTACGT"), (["-a", "XACGTACGT"], "XACGTACGT"),
           (["-g", "ACGTACGT$"], "ACGTACGT$"), (["-g", "ACGTACGTX"], "ACGTACGTX"),
           (["-g", "^XACGTACGT"], "^XACGTACGT"), (["-a", "ACGTACGTX$"], "ACGTACGTX$"),
           (["-g", "^ACGTACGT...TTGGCCAA"], "linked"), (["-g", "ACGTACGT...TTGGCCAA$"], "linked")]


@pytest.mark.parametrize("args,needle", REFUSED)
def test_refused_specs_exit_with_status_2(tmp_path, capsys, args, needle):
    """As cutadapt refuses them; anchors inside a linked adapter are out of scope.  The refusal
    comes before the input or a device is opened."""
    with pytest.raises(SystemExit) as ei:
        cli.run(args + ["-o", str(tmp_path / "o.fastq"), str(tmp_path / "missing.fastq")])
    assert ei.value.code == 2
    err = capsys.readouterr().err
    assert "error:" in err and needle in err


def test_still_out_of_scope_exit_with_status_2(tmp_path):
    for extra in (["--no-indels"], ["-b", "ACGTACGT"]):
        with pytest.raises(SystemExit) as ei:
            cli.run(["-g", "^ACGTACGT"] + extra + ["-o", str(tmp_path / "o.fq"),
                                                  str(tmp_path / "missing.fq")])
        assert ei.value.code == 2


def test_report_type_strings():
    ads = _parse(("front", "^ACGTACGTAC"), ("front", "XACGTACGTAC"), ("back", "ACGTACGTAC$"),
                 ("back", "ACGTACGTACX"), ("front", "ACGTACGTAC"), ("back", "ACGTACGTAC"))
    st = Stats(ads)
    js = st.to_json(argv=[], cores=1, in_path="x", error_rate=0.1)
    types = [(a["five_prime_end"] or a["three_prime_end"])["type"] for a in js["adapters_read1"]]
    assert types[:4] == ["anchored_five_prime", "noninternal_five_prime",
                         "anchored_three_prime", "noninternal_three_prime"]
    assert all(t.startswith("regular") for t in types[4:])
    assert [a["five_prime_end"] is None for a in js["adapters_read1"]] == \
        [False, False, True, True, False, True]


def _render(records, exp, wheres, names, demux):
    """Output name -> records, as cutadapt writes them for the oracle's results."""
    out = {}
    for (name, seq, qual), r in zip(records, exp):
        if r["rc1"]:
            seq, qual, name = ec.revcomp(seq), qual[::-1], name + " rc"
        b = int(r["bin1"])
        if b >= 0 and wheres[b] & ec.F:
            seq, qual = seq[r["m1_rstop"]:], qual[r["m1_rstop"]:]
        elif b >= 0:
            seq, qual = seq[:r["m1_rstart"]], qual[:r["m1_rstart"]]
        key = (names[b] if b >= 0 else "unknown") if demux else ("out" if b >= 0 else "untrimmed")
        out.setdefault(key, []).append(("@" + name, seq, qual))
    return out


@pytest.mark.gpu
def test_dropin_end_to_end(tmp_path):
    """`cutadapt -g ^file:… --rc -o {name}.fastq --json` and a literal mixed call with
    --untrimmed-output: every output file equals the oracle's records, the JSON carries the
    types and the per-adapter totals."""
    rng = np.random.default_rng(99)
    bcs = [ec._rand(rng, 24) for _ in range(6)]
    names = [f"BC{i + 1:02d}" for i in range(6)]
    fa = tmp_path / "barcodes.fa"
    fa.write_text("".join(f">{n} demo\n{s}\n" for n, s in zip(names, bcs)))
    seqs = []
    for i in range(1500):
        r = ec._sub(rng, bcs[i % 6], int(rng.integers(0, 4))) + ec._rand(rng, 60 + i % 200)
        if i % 9 == 0:
            r = ec._rand(rng, 12) + r          # the barcode is internal: ^ must not take it
        seqs.append(ec.revcomp(r) if i % 3 == 0 else r)
    recs = [(f"r{i} ch={i % 7}", s, q)
            for i, (s, q) in enumerate(zip(seqs, random_quals(rng, [len(s) for s in seqs])))]
    infile = str(tmp_path / "in.fastq")
    write_fastq(infile, *zip(*recs))
    js = tmp_path / "r.json"
    subprocess.run([CLI, "-e", "0.1", "--rc", "-g", f"^file:{fa}", "-o",
                    str(tmp_path / "{name}.fastq"), f"--json={js}", infile], check=True,
                   stdout=subprocess.DEVNULL)
    wheres = [ec.PREFIX] * 6
    exp = ec.demux(bcs, wheres, seqs, True, 0.1, 3)
    want = _render(recs, exp, wheres, names, True)
    assert len(want["unknown"]) > 150 and all(len(want[n]) > 100 for n in names)
    for key in names + ["unknown"]:
        assert read_fastq(str(tmp_path / f"{key}.fastq")) == want.get(key, []), key
    rep = json.loads(js.read_text())
    assert [a["five_prime_end"]["type"] for a in rep["adapters_read1"]] == \
        ["anchored_five_prime"] * 6
    assert [a["total_matches"] for a in rep["adapters_read1"]] == [len(want[n]) for n in names]

    # literal specs of four types in one call, no {name}: trimmed to -o, the rest untrimmed
    # (reads 0 and 3 mod 6 were written reverse-complemented: their barcodes end the read)
    ads = [("-g", "X" + bcs[1], ec.FRONTX), ("-a", ec.revcomp(bcs[0]) + "$", ec.SUFFIX),
           ("-g", bcs[2], ec.F), ("-a", ec.revcomp(bcs[3]) + "X", ec.BACKX)]
    cmd = [CLI, "-e", "0.15", "-O", "5"]
    for flag, spec, _ in ads:
        cmd += [flag, spec]
    out, unt = tmp_path / "trimmed.fastq", tmp_path / "untrimmed.fastq"
    subprocess.run(cmd + ["-o", str(out), f"--untrimmed-output={unt}", infile], check=True,
                   stdout=subprocess.DEVNULL)
    aseq = [bcs[1], ec.revcomp(bcs[0]), bcs[2], ec.revcomp(bcs[3])]
    wh = [w for _, _, w in ads]
    exp = ec.demux(aseq, wh, seqs, False, 0.15, 5)
    want = _render(recs, exp, wh, None, False)
    assert len(want["out"]) > 300 and len(want["untrimmed"]) > 300
    assert len({int(b) for b in exp["bin1"]}) == 5
    assert read_fastq(str(out)) == want["out"]
    assert read_fastq(str(unt)) == want["untrimmed"]


@pytest.mark.gpu
def test_demux_loop_takes_the_markers_of_its_panel_files(tmp_path):
    """dmx-demux-loop with `^SEQ` records in --sp5 and `SEQ$` records in --sp27 (the fused
    two-round mode, `^` in round 0 and `$` anchored at the trimmed read's end in round 1) writes
    per (SP5, SP27) bin what the two rounds of drop-in calls write; a read whose barcode is
    internal stays out of every bin."""
    from helpers import LOOP
    rng = np.random.default_rng(5)
    b5 = [ec._rand(rng, 22) for _ in range(3)]
    b27 = [ec._rand(rng, 20) for _ in range(3)]
    n5, n27 = [f"F{i}" for i in range(3)], [f"R{i}" for i in range(3)]
    f5, f27 = tmp_path / "sp5.fa", tmp_path / "sp27.fa"
    f5.write_text("".join(f">{n}\n^{s}\n" for n, s in zip(n5, b5)))
    f27.write_text("".join(f">{n}\n{s}$\n" for n, s in zip(n27, b27)))
    seqs = []
    for i in range(900):
        r = ec._sub(rng, b5[i % 3], i % 3) + ec._rand(rng, 80 + i % 90) + \
            ec._sub(rng, b27[(i // 3) % 3], i % 2)
        if i % 10 == 0:
            r = ec._rand(rng, 9) + r            # round 0's barcode is internal
        if i % 11 == 0:
            r = r + ec._rand(rng, 9)            # round 1's is
        seqs.append(ec.revcomp(r) if i % 4 == 0 else r)
    names = [f"r{i}" for i in range(len(seqs))]
    infile = tmp_path / "pychopped" / "pychopped_ds7.fastq"
    infile.parent.mkdir()
    write_fastq(str(infile), names, seqs, random_quals(rng, [len(s) for s in seqs]))
    od = tmp_path / "loop"
    subprocess.run([LOOP, str(infile), "-j", "2", "--outdir", str(od), "--sp5", str(f5),
                    "--sp27", str(f27)], check=True, stdout=subprocess.DEVNULL)
    r1 = tmp_path / "r1"
    r1.mkdir()
    subprocess.run([CLI, "-e", "0.1", "--rc", "-g", f"file:{f5}", "-o",
                    str(r1 / "{name}.fastq"), str(infile)], check=True,
                   stdout=subprocess.DEVNULL)
    total = 0
    for a in n5:
        subprocess.run([CLI, "-e", "0.1", "--rc", "-a", f"file:{f27}", "-o",
                        str(r1 / ("{name}_" + a + ".fastq")), str(r1 / f"{a}.fastq")],
                       check=True, stdout=subprocess.DEVNULL)
        for b in n27:
            want = read_fastq(str(r1 / f"{b}_{a}.fastq"))
            assert read_fastq(f"{od}/SP27/{b}_{a}_ds7.fastq.gz") == want, (a, b)
            total += len(want)
    assert 500 < total < 800   # the internal-barcode reads (about 1 in 5) are in no bin


def test_demux_loop_refuses_a_marker_on_the_wrong_panel(tmp_path, capsys):
    from dmx import loop
    fq = tmp_path / "pychopped_x.fastq"
    fq.write_text("@r1\nACGTACGTACGT\n+\nIIIIIIIIIIII\n")
    bad = tmp_path / "sp5.fa"
    bad.write_text(">a\nACGTACGTAC$\n")
    assert loop.run([str(fq), "--outdir", str(tmp_path / "o"), "--sp5", str(bad)]) == 2
    assert "ACGTACGTAC$" in capsys.readouterr().err
