"""CPU: the draws of a batched TTA call.  The reference draws per face, in face order, three values per copy from Python's
global `random` (deepfake_detection.py:419-426).  A fused call does not know its face count in advance, so
`tta_draw_table` draws for the call's capacity and `tta_commit_draws` rewinds and re-draws the rows that were used: the
first rows equal the reference's loop and the global stream ends where that loop would have left it."""
import random

import pytest


def _reference_loop(faces, copies):
    rows = []
    for _ in range(faces):
        for _ in range(copies):
            flip = random.random() > 0.5
            brightness = random.uniform(0.9, 1.1)
            angle = random.uniform(-3, 3)
            rows.append((flip, brightness, angle))
    return rows


@pytest.mark.parametrize("faces,copies", [(0, 2), (3, 2), (8, 1), (8, 3)])
def test_draw_table_and_commit_follow_the_reference_stream(pkg, faces, copies):
    D = pkg.deepfake_detection
    random.seed(4321)
    start = random.getstate()
    want = _reference_loop(faces, copies)
    want_state = random.getstate()
    random.seed(4321)
    state, table = D.tta_draw_table(8, copies)
    assert state == start and len(table) == 8 * copies
    assert table[: faces * copies] == want
    assert all(isinstance(f, bool) and 0.9 <= b <= 1.1 and -3 <= a <= 3 for f, b, a in table)
    if faces < 8:
        assert random.getstate() != want_state              # the table drew past the used rows
    D.tta_commit_draws(state, faces, copies)
    assert random.getstate() == want_state
    if faces == 0:
        assert random.getstate() == start                   # a call without faces leaves the stream untouched


def test_next_call_continues_where_the_used_rows_end(pkg):
    """two calls in a row (2 faces, then 1) give the rows of one reference loop over 3 faces"""
    D = pkg.deepfake_detection
    random.seed(99)
    want = _reference_loop(3, 2)
    random.seed(99)
    s1, t1 = D.tta_draw_table(8, 2)
    D.tta_commit_draws(s1, 2, 2)
    s2, t2 = D.tta_draw_table(8, 2)
    D.tta_commit_draws(s2, 1, 2)
    assert t1[:4] + t2[:2] == want
