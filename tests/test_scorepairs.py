"""oavif_amd.scorepairs without a GPU: grouping by size, batches of at most B, rows in input order, bad lines reported
with their line number.  The scorer is a fake whose score of a pair is a function of the two frames alone."""
import csv
import io
import os

import numpy as np
import pytest

from oavif_amd import pam, scorepairs


class FakeScorer:
    def __init__(self):
        self.calls = []

    def score_batch(self, refs, dists):
        assert len(refs) == len(dists) and len({r.shape for r in refs} | {d.shape for d in dists}) == 1
        self.calls.append((refs[0].shape, len(refs)))
        return np.array([float(int(r[0, 0, 0]) * 1000 + int(d[0, 0, 0])) for r, d in zip(refs, dists)])


def _frame(w, h, tag):
    a = np.zeros((h, w, 3), np.uint8)
    a[0, 0, 0] = tag
    return a


def _write_pairs(tmp_path, specs):
    """specs: [(w, h)] -> the pair list's text; pair k holds tags 2k / 2k + 1 in its first pixel."""
    lines = []
    for k, (w, h) in enumerate(specs):
        for tag, name in ((2 * k, f"r{k}.pam"), (2 * k + 1, f"d{k}.pam")):
            (tmp_path / name).write_bytes(pam.write_pam(_frame(w, h, tag)))
        lines.append(f"r{k}.pam\td{k}.pam")
    return lines


def test_groups_by_size_batches_and_keeps_input_order(tmp_path):
    specs = [(16, 8), (32, 8), (16, 8), (16, 8), (9, 9), (16, 8), (32, 8), (16, 8), (16, 8)]
    lines = _write_pairs(tmp_path, specs)
    text = "# a corpus\n" + "\n".join(lines[:4]) + "\n\n" + "\n".join(lines[4:]) + "\n"
    pairs = scorepairs.parse_pairs(text, str(tmp_path))
    assert [p[0] for p in pairs] == [2, 3, 4, 5, 7, 8, 9, 10, 11]          # 1-based lines, comment and blank skipped
    fake = FakeScorer()
    rows = scorepairs.score_pairs(fake, pairs, batch=4)
    # six 16x8 pairs -> batches of 4 and 2 (a group larger than B), two 32x8 pairs, one 9x9 pair (a group of one)
    assert sorted(fake.calls) == sorted([((8, 16, 3), 4), ((8, 16, 3), 2), ((8, 32, 3), 2), ((9, 9, 3), 1)])
    assert [r[0] for r in rows] == [p[0] for p in pairs]
    for k, row in enumerate(rows):
        line, rp, dp, w, h, score = row
        assert (w, h) == specs[k] and os.path.basename(rp) == f"r{k}.pam" and os.path.basename(dp) == f"d{k}.pam"
        assert score == 2 * k * 1000 + 2 * k + 1                                # each pair's own score, in input order
    out = io.StringIO()
    scorepairs.write_csv(rows, out)
    got = list(csv.reader(io.StringIO(out.getvalue())))
    assert got[0] == ["line", "ref", "dist", "width", "height", "score"] and len(got) == 1 + len(specs)
    assert [float(r[5]) for r in got[1:]] == [r[5] for r in rows]


def test_one_batch_when_b_is_large_and_b_of_one(tmp_path):
    lines = _write_pairs(tmp_path, [(16, 8)] * 3)
    pairs = scorepairs.parse_pairs("\n".join(lines), str(tmp_path))
    fake = FakeScorer()
    scorepairs.score_pairs(fake, pairs, batch=64)
    assert fake.calls == [((8, 16, 3), 3)]
    fake = FakeScorer()
    rows = scorepairs.score_pairs(fake, pairs, batch=1)
    assert fake.calls == [((8, 16, 3), 1)] * 3 and [r[5] for r in rows] == [1.0, 2003.0, 4005.0]
    with pytest.raises(ValueError):
        scorepairs.score_pairs(fake, pairs, batch=0)


def test_a_missing_file_is_reported_with_its_line(tmp_path):
    lines = _write_pairs(tmp_path, [(16, 8), (16, 8)])
    text = lines[0] + "\n\n" + "r1.pam\tnowhere.pam\n"
    pairs = scorepairs.parse_pairs(text, str(tmp_path))
    fake = FakeScorer()
    with pytest.raises(scorepairs.PairListError) as ei:
        scorepairs.score_pairs(fake, pairs, batch=4)
    assert ei.value.line == 3 and "nowhere.pam" in str(ei.value) and "line 3" in str(ei.value)
    assert fake.calls == []                                                      # nothing scored before the report
    tsv = tmp_path / "pairs.tsv"
    tsv.write_text(text)
    assert scorepairs.main([str(tsv), str(tmp_path / "out.csv")], scorer=fake) == 1
    assert not (tmp_path / "out.csv").exists()


def test_bad_lines_and_mismatched_sizes(tmp_path):
    with pytest.raises(scorepairs.PairListError) as ei:
        scorepairs.parse_pairs("a.pam\tb.pam\nonly_one_column\n", str(tmp_path))
    assert ei.value.line == 2
    (tmp_path / "a.pam").write_bytes(pam.write_pam(_frame(16, 8, 1)))
    (tmp_path / "b.pam").write_bytes(pam.write_pam(_frame(8, 16, 2)))
    with pytest.raises(scorepairs.PairListError) as ei:
        scorepairs.score_pairs(FakeScorer(), scorepairs.parse_pairs("a.pam\tb.pam", str(tmp_path)))
    assert ei.value.line == 1 and "16x8" in str(ei.value)
    (tmp_path / "c.jpg").write_bytes(b"x")
    with pytest.raises(scorepairs.PairListError):
        scorepairs.score_pairs(FakeScorer(), scorepairs.parse_pairs("a.pam\tc.jpg", str(tmp_path)))


def test_main_writes_the_csv(tmp_path):
    lines = _write_pairs(tmp_path, [(16, 8), (9, 9), (16, 8)])
    tsv = tmp_path / "pairs.tsv"
    tsv.write_text("\n".join(lines) + "\n")
    fake = FakeScorer()
    assert scorepairs.main([str(tsv), str(tmp_path / "out.csv"), "--batch", "8"], scorer=fake) == 0
    got = list(csv.reader(open(tmp_path / "out.csv")))
    assert [r[0] for r in got[1:]] == ["1", "2", "3"] and [float(r[5]) for r in got[1:]] == [1.0, 2003.0, 4005.0]
    assert scorepairs.main([str(tsv)], scorer=fake) == 2
