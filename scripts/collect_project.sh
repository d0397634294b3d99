#!/bin/bash
# Concatenate the project's sources and docs into one text file for review (the
# reference's collect_project.sh / collect_p_docs.sh). usage: scripts/collect_project.sh [OUT]
set -euo pipefail
cd "$(dirname "$0")/.."
out="${1:-project.txt}"
list_files() {  # the tracked sources; in an exported tree (no .git) the same patterns from the file system
  if git rev-parse --is-inside-work-tree > /dev/null 2>&1; then
    git ls-files 'README.md' 'docs/*.md' 'CMakeLists.txt' 'csrc/**' 'cuda-mpi-gpu-cluster-programming_amd/**/*.py' \
      '*.py' 'tools/*.py' 'scripts/*.sh' 'tests/*.py'
  else
    { ls README.md CMakeLists.txt docs/*.md ./*.py tools/*.py scripts/*.sh tests/*.py 2>/dev/null
      find csrc -type f ! -name '*.o'
      find cuda-mpi-gpu-cluster-programming_amd -type f -name '*.py'; } | sed 's|^\./||' | LC_ALL=C sort -u
  fi
}
{
  echo "# anx project dump — $(git rev-parse --short HEAD 2>/dev/null || echo nogit) — $(date -u +%F)"
  list_files | while read -r f; do
    echo
    echo "===== $f ($(wc -l < "$f") lines) ====="
    cat "$f"
  done
} > "$out"
echo "wrote $out ($(wc -l < "$out") lines)"
