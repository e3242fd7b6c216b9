"""The cache tag of the CPU models' loader (tests/c_model.py: build_tag) covers every file the build reads: the source, the
headers it includes and the headers those include, and the command.  Nothing is compiled here."""
from __future__ import annotations

import pytest

from tests.c_model import build_tag

CMD = ["cc", "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-lm"]


@pytest.fixture()
def tree(tmp_path):
    """model.c includes shared.h, which includes inner.h from a directory of its own; nothing includes lonely.h; <math.h> is
    the system's."""
    (tmp_path / "sub").mkdir()
    (tmp_path / "model.c").write_text('#include <math.h>\n#include "shared.h"\nint f(void) { return G + 1; }\n')
    (tmp_path / "shared.h").write_text('  #  include "sub/inner.h"\n#define G (INNER + 1)\n')
    (tmp_path / "sub" / "inner.h").write_text("#define INNER 1\n")
    (tmp_path / "lonely.h").write_text("#define LONELY 1\n")
    return tmp_path


def _tag(tree, cmd=CMD):
    return build_tag(str(tree / "model.c"), cmd)


def test_the_tag_is_a_function_of_what_the_build_reads(tree):
    assert _tag(tree) == _tag(tree) and len(_tag(tree)) == 12


@pytest.mark.parametrize("edited", ["model.c", "shared.h", "sub/inner.h"])
def test_an_edit_to_the_source_or_to_a_header_it_reaches_changes_the_tag(tree, edited):
    before = _tag(tree)
    with open(tree / edited, "a") as f:
        f.write("/* edited */\n")
    assert _tag(tree) != before


def test_a_file_that_nothing_includes_does_not_change_the_tag(tree):
    before = _tag(tree)
    (tree / "lonely.h").write_text("#define LONELY 2\n")
    (tree / "math.h").write_text("#define NOT_THE_SYSTEMS 1\n")      # <math.h> is not followed to a file next to the source
    assert _tag(tree) == before


def test_two_sets_of_flags_have_two_tags(tree):
    assert _tag(tree) != _tag(tree, CMD[:-1] + ["-DMUTANT_X", "-lm"])
    assert _tag(tree, CMD + ["-DMUTANT_X"]) != _tag(tree, CMD + ["-DMUTANT_Y"])


def test_headers_that_include_each_other_end(tree):
    (tree / "sub" / "inner.h").write_text('#include "../shared.h"\n#define INNER 1\n')
    assert len(_tag(tree)) == 12
