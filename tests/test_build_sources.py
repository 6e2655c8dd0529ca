"""build.SOURCES against phyx_amd/csrc: build._sources() skips a listed file that is missing, and the shared link accepts undefined
symbols, so a translation unit that is forgotten (or misspelt) would surface only when one of its functions is first called."""
import os

from phyx_amd import build


def test_every_translation_unit_is_listed_and_exists():
    on_disk = sorted(f for f in os.listdir(build.CSRC) if f.endswith(".hip"))
    assert len(build.SOURCES) == len(set(build.SOURCES)), "a file is listed twice"
    assert sorted(build.SOURCES) == on_disk
    assert set(build.FILE_FLAGS) <= set(build.SOURCES), "per-file flags for a file that is not built"
