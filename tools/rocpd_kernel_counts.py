"""Kernel names (in full) and call counts of a rocprofv3 `--kernel-trace` SQLite database (rocpd format), sorted by name."""
import sqlite3
import sys

rows = sqlite3.connect(sys.argv[1]).execute("select name, count(*) from kernels group by name order by name").fetchall()
for name, n in rows:
    print("%7d  %s" % (n, name))
print("%7d  TOTAL (%d kernels)" % (sum(n for _, n in rows), len(rows)))
