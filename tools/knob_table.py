#!/usr/bin/env python3
"""Every DNE_* environment knob the engine reads: the rows of KNOBS in csrc/plan.h ({name, lo, hi, &Knobs::field, "what it selects"}) with the
field's initialiser in struct Knobs as the default -- printed as the markdown table of DESIGN.md's knob appendix (section 11).
python tools/knob_table.py > /tmp/knobs.md"""
import os, re
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
src = open(os.path.join(ROOT, "deep-neuroevolution_amd", "csrc", "plan.h")).read()
struct = re.search(r"struct Knobs \{(.*?)\n\};", src, re.S).group(1)
defaults = dict(re.findall(r"(\w+) = ([^,;]+)", struct))
print("| knob | default | range | what it selects |")
print("|---|---|---|---|")
for name, lo, hi, field, text in sorted(re.findall(r'\{"(DNE_\w+)", ([^,]+), ([^,]+), &Knobs::(\w+), "(.*)"\},', src)):
    print("| `%s` | %s | %s .. %s | %s |" % (name, defaults[field], lo, hi, text.replace("|", "\\|")))
