"""ancient_contig_merge on the device against the directed cases (tests/contigcases.py), through the C ABI in one process with one
context (the device queue's 1.3 GB tables are filled once): every set with the queue on the device and on the host - sequences and
ext flags against the oracle and against the reference's committed output, the device's own account of its rounds (CDM_TIMING)
against the oracle's event log -, the launches cut into slices, --unsafe 1, the queries the device hands back, the case it refuses,
and two rows through the module binary."""
import os
import re
import subprocess

import pytest

import contigcases as cc
from carpedeam_amd import capi, mmdb
from contigcases import fixture
from gpuutil import diff_keys, seqdb_to_keyed

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [n for n, _, _ in cc.SETS]
SWITCHES = ("CDM_CONTIG_QUEUE", "CDM_CONTIG_HAND_BACK_EVERY", "CDM_LAUNCH_SLICE", "CDM_TIMING")
SUMMARY = re.compile(r"contig merge: (\d+) rounds, (\d+) growths, (\d+) parked hits re-aligned, (\d+) queries handed back to the host")


@pytest.fixture(scope="module")
def ctx(dhigh_prefix):
    c = capi.Ctx(0)
    c.damage_load(dhigh_prefix)
    return c


@pytest.fixture(scope="module")
def expected(oracle_bin, dhigh_prefix, tmp_path_factory):
    """per set: the case set, the oracle's output and event log on the committed inputs, the reference's committed output, --max-seq-len"""
    d = tmp_path_factory.mktemp("gpu_contig_directed")
    out = {}
    for name, make, max_seq_len in cc.SETS:
        merged, events = cc.run_oracle_on_fixture(oracle_bin, dhigh_prefix, d, name, max_seq_len)
        out[name] = (make(), merged, events, fixture(name, "cmerge"), max_seq_len)
    return out


def switches(monkeypatch, **env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    capi.lib()                                                   # the library reads its switches again


def broken_groups(S, bad_keys):
    by_key = {g["key"]: g["name"] for g in S.groups}
    return sorted({by_key.get(k, "target %d of no group" % k) for k in bad_keys})


def device_merge(ctx, seq_keyed, aln_keyed, max_seq_len=200000, unsafe=0, min_cov=5):
    par = capi.AncientParams.default()
    par.max_seq_len, par.unsafe, par.min_cov_safe = max_seq_len, unsafe, min_cov
    db = ctx.upload_keyed_seqdb(seq_keyed)
    _, keys, _ = db.meta()
    off, rec = capi.parse_aln_db(aln_keyed, keys)
    return seqdb_to_keyed(*ctx.contig_merge(db, ctx.upload_alns(db, off, rec), par).download())


def summary_line(capfd):
    """(rounds, growths, parked hits re-aligned, queries handed back) of the device queue's last call"""
    found = SUMMARY.findall(capfd.readouterr().err)
    assert len(found) == 1, found
    return tuple(int(x) for x in found[0])


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("name", NAMES)
def test_directed_cases_match_oracle_and_reference(ctx, expected, monkeypatch, capfd, name, where):
    """The summary line against the oracle's event log (contigcases.device_totals holds the mapping, derived from cqRound and the
    loop of cdm_contig_queue_device): a query's device rounds are its logged rounds plus one where its last logged round parked hits
    on an empty queue (the device finds out that none passed in a round of its own); growths are the (query, round) pairs with an
    offset; parked hits are those of rounds that end on an empty queue; no letter beyond ACGTN in these sets, so nothing is handed back."""
    switches(monkeypatch, CDM_CONTIG_QUEUE=where, CDM_TIMING=1)
    S, oracle, events, reference, max_seq_len = expected[name]
    capfd.readouterr()
    got = device_merge(ctx, fixture(name, "corr"), fixture(name, "aln"), max_seq_len)
    bad = diff_keys(got, oracle)
    assert not bad, "%s queue: differs from the oracle in groups %s" % (where, broken_groups(S, bad))
    bad = diff_keys(got, reference)
    assert not bad, "%s queue: differs from the reference in groups %s" % (where, broken_groups(S, bad))
    if where == "device":
        assert summary_line(capfd) == cc.device_totals(events) + (0,), "set %s: the device queue's rounds, growths, parked hits and hand-backs against the oracle's log" % name
    else:
        assert "queues + extension (host)" in capfd.readouterr().err


@pytest.mark.parametrize("name", ["rounds", "letters"])
def test_sliced_launches(ctx, expected, monkeypatch, name):
    """CDM_LAUNCH_SLICE=7: the statistics, the grown queries, the parked hits and the gather in launches of seven items"""
    switches(monkeypatch, CDM_CONTIG_QUEUE="device", CDM_LAUNCH_SLICE=7)
    S, oracle, _, reference, max_seq_len = expected[name]
    got = device_merge(ctx, fixture(name, "corr"), fixture(name, "aln"), max_seq_len)
    bad = diff_keys(got, reference)
    assert not bad, "sliced launches: differs from the reference in groups %s" % broken_groups(S, bad)
    assert not diff_keys(got, oracle)


@pytest.mark.parametrize("every", [1, 2])
@pytest.mark.parametrize("name", cc.MAIN)
def test_main_groups_handed_back(ctx, expected, monkeypatch, capfd, name, every):
    """CDM_CONTIG_HAND_BACK_EVERY: every query (every second one) goes the way of a comparison too close to call"""
    switches(monkeypatch, CDM_CONTIG_QUEUE="device", CDM_CONTIG_HAND_BACK_EVERY=every, CDM_TIMING=1)
    S, oracle, events, reference, max_seq_len = expected[name]
    capfd.readouterr()
    got = device_merge(ctx, fixture(name, "corr"), fixture(name, "aln"), max_seq_len)
    bad = diff_keys(got, reference)
    assert not bad, "hand back every %d: differs from the reference in groups %s" % (every, broken_groups(S, bad))
    # the active queries (those with a gated record) whose index is a multiple of `every`; keys are indices in these sets
    assert summary_line(capfd)[3] == sum(1 for k, e in events.items() if e.gated and k % every == 0)


@pytest.mark.parametrize("min_cov", [1, 2, 5])
@pytest.mark.parametrize("name", cc.MAIN)
def test_main_sets_unsafe_mode_matches_oracle(ctx, oracle_bin, dhigh_prefix, tmp_path, monkeypatch, name, min_cov):
    """--unsafe 1 against the oracle (whose unsafe mode tests/test_contig_directed.py holds against a live run of the reference where
    that is built).  The generator's own filter takes out what the device refuses: nothing of these sets, a share of 0 - below a
    quarter; that the filtered sets still hold every group is checked on the CPU (test_unsafe_filter_keeps_the_set)."""
    switches(monkeypatch, CDM_CONTIG_QUEUE="device")
    S = dict((n, m) for n, m, _ in cc.SETS)[name]()
    seq_keyed, aln_keyed, refused = cc.without_unsupported(S)
    assert refused < len(S.groups) / 4
    exp, _ = cc.run_oracle_on(oracle_bin, dhigh_prefix, tmp_path, name, seq_keyed, aln_keyed, 200000, 1, min_cov)
    got = device_merge(ctx, seq_keyed, aln_keyed, 200000, 1, min_cov)
    bad = diff_keys(got, exp)
    assert not bad, "unsafe, min-cov-safe %d: differs from the oracle in groups %s" % (min_cov, broken_groups(S, bad))
    assert sum(v[1] for v in exp.values()) > 0                       # (something grows in this mode)


@pytest.mark.parametrize("where", ["device", "host"])
def test_letters_beyond_acgtn(ctx, oracle_bin, dhigh_prefix, tmp_path, monkeypatch, capfd, where):
    """the handback set: a query with IUPAC or lower-case letters is handed back in round 0 (SeqMeta flag 4 of the query), and so is a
    query that pops a target with such letters - cqRound looks at the target's flag before it parks a hit, and every record is popped
    in the round that queues it first, so this is round 0 as well, although the reference uses that target in its second round only:
    four queries"""
    switches(monkeypatch, CDM_CONTIG_QUEUE=where, CDM_TIMING=1)
    S = cc.handback_set()
    exp, _ = cc.run_oracle_on(oracle_bin, dhigh_prefix, tmp_path, "handback", S.seq_keyed(), S.aln_keyed(), 200000)
    capfd.readouterr()
    got = device_merge(ctx, S.seq_keyed(), S.aln_keyed())
    bad = diff_keys(got, exp)
    assert not bad, "%s queue: differs from the oracle in groups %s" % (where, broken_groups(S, bad))
    if where == "device":
        assert summary_line(capfd)[3] == 4


def test_arguments_beyond_the_tables_go_back_to_the_host(ctx, oracle_bin, dhigh_prefix, tmp_path, monkeypatch, capfd):
    """two overlaps of more than 2^18 columns: xHit + yHit >= 2^19 leaves lgammaf's table, the query is handed back"""
    switches(monkeypatch, CDM_CONTIG_QUEUE="device", CDM_TIMING=1)
    S = cc.tables_set()
    exp, _ = cc.run_oracle_on(oracle_bin, dhigh_prefix, tmp_path, "tables", S.seq_keyed(), S.aln_keyed(), cc.TABLES_MAX_SEQ_LEN)
    capfd.readouterr()
    got = device_merge(ctx, S.seq_keyed(), S.aln_keyed(), cc.TABLES_MAX_SEQ_LEN)
    bad = diff_keys(got, exp)
    assert not bad, "differs from the oracle in groups %s" % broken_groups(S, bad)
    assert summary_line(capfd)[3] >= 1
    assert len(mmdb.canon(exp)[0][0]) > cc.TABLES_QLEN                 # (it grew)


@pytest.mark.parametrize("where", ["device", "host"])
def test_overhang_beyond_the_query_is_refused(ctx, oracle_bin, dhigh_prefix, tmp_path, monkeypatch, where):
    """a target that overhangs its query by qLen + 1 letters: CDM_ERR_UNSUPPORTED (-4) from the device queue and from the host code
    alike (k_cq_gate's counter 0; host/contigmerge.cpp's undefinedCase) - the reference pads with a negative number of letters there.
    At exactly qLen the call goes through and equals the oracle"""
    switches(monkeypatch, CDM_CONTIG_QUEUE=where)
    S = cc.refusal_set(1)
    with pytest.raises(capi.CdmError, match=r"cdm error -4: .*overhangs its query by more than the query's length"):
        device_merge(ctx, S.seq_keyed(), S.aln_keyed())
    S = cc.refusal_set(0)
    exp, _ = cc.run_oracle_on(oracle_bin, dhigh_prefix, tmp_path, "refusal", S.seq_keyed(), S.aln_keyed(), 200000)
    got = device_merge(ctx, S.seq_keyed(), S.aln_keyed())
    assert not diff_keys(got, exp)
    assert len(mmdb.canon(got)[0][0]) == 240 and mmdb.canon(got)[0][1] == 1


@pytest.mark.parametrize("name,unsafe,min_cov,queue", [("rounds", 0, 5, None), ("gates", 1, 2, "device")])
def test_module_binary_on_db_files(oracle_bin, dhigh_prefix, tmp_path, monkeypatch, name, unsafe, min_cov, queue):
    """`carpedeam ancient_contig_merge` on DB files: the default of a module process (the host queue, no tables) against the reference's
    output, and --unsafe 1 --min-cov-safe 2 with the queue pinned to the device against the oracle"""
    from carpedeam_amd import build
    build.build()
    switches(monkeypatch, **({"CDM_CONTIG_QUEUE": queue} if queue else {}))
    exe = os.path.join(ROOT, "carpedeam_amd", "carpedeam")
    t = lambda s: str(tmp_path / s)
    mmdb.write_from_keyed(t("corr"), fixture(name, "corr"), mmdb.DBTYPE_NUCLEOTIDES)
    mmdb.write_from_keyed(t("aln"), fixture(name, "aln"), mmdb.DBTYPE_ALIGNMENT_RES)
    r = subprocess.run([exe, "ancient_contig_merge", t("corr"), t("aln"), t("out"), *cc.flags_for(200000, unsafe, min_cov), "--ancient-damage", dhigh_prefix, "--threads", "4"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-1000:]
    if unsafe:
        exp, _ = cc.run_oracle_on(oracle_bin, dhigh_prefix, tmp_path, name, fixture(name, "corr"), fixture(name, "aln"), 200000, unsafe, min_cov)
    else:
        exp = fixture(name, "cmerge")
    S = dict((n, m) for n, m, _ in cc.SETS)[name]()
    bad = diff_keys(mmdb.read_db(t("out")), exp)
    assert not bad, "module binary: differs in groups %s" % broken_groups(S, bad)
