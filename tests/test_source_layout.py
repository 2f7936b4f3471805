"""The layout of csrc/: no file includes another unit's source, and every *.hip there is exactly one object of the Makefile.
Kernels that two units instantiate are templates in headers (rt_whitted_kernel.h, rt_pwf_kernel.h, rt_dist_kernels.h, rt_rng.h, rt_atrous_kernel.h,
rt_film_splat_kernel.h); the launch shape the image-side units share is rt_image_kernel.h.
Pure text: needs no build."""
import re
from pathlib import Path

CSRC = Path(__file__).resolve().parent.parent / "homework-18-graphics-raytracer_amd" / "csrc"


def _makefile_list(name: str):
    """the words of `NAME = ...` in the Makefile (continuation lines joined)"""
    text = (CSRC / "Makefile").read_text().replace("\\\n", " ")
    found = re.findall(rf"^{name}\s*=(.*)$", text, flags=re.M)
    assert len(found) == 1, (name, found)
    return found[0].split()


def test_no_file_includes_a_hip_source():
    sources = sorted(p for pattern in ("*.hip", "*.h", "*.inc") for p in CSRC.rglob(pattern))
    assert sources
    bad = []
    for path in sources:
        for number, line in enumerate(path.read_text().splitlines(), 1):
            m = re.match(r'\s*#\s*include\s*[<"]([^>"]+)[>"]', line)
            if m and m.group(1).endswith(".hip"):
                bad.append(f"{path.relative_to(CSRC)}:{number}: {line.strip()}")
    assert not bad, bad


def test_every_hip_is_one_unit_of_the_makefile():
    objs = _makefile_list("KERNEL_OBJS")
    assert all(o.endswith(".o") for o in objs), objs
    listed = [o[:-2] + ".hip" for o in objs] + _makefile_list("API_SRCS")
    assert all(name.endswith(".hip") for name in listed), listed
    on_disk = sorted(p.name for p in CSRC.glob("*.hip"))
    assert sorted(listed) == on_disk, (sorted(set(listed) ^ set(on_disk)), sorted(n for n in set(listed) if listed.count(n) > 1))
