"""Lines of code of Python files, now or at a git revision: non-blank lines that hold anything but comments and docstrings.
``python tools/count_code_lines.py [--rev REV] FILE...`` prints one count per file and their sum (a file that does not exist counts 0)."""
import argparse
import ast
import io
import os
import subprocess
import tokenize


def code_lines(src: str) -> int:
    doc = set()
    for n in ast.walk(ast.parse(src)):
        if isinstance(n, (ast.Module, ast.ClassDef, ast.FunctionDef, ast.AsyncFunctionDef)) and n.body and isinstance(n.body[0], ast.Expr) \
                and isinstance(n.body[0].value, ast.Constant) and isinstance(n.body[0].value.value, str):
            doc.update(range(n.body[0].lineno, n.body[0].end_lineno + 1))
    skip = (tokenize.COMMENT, tokenize.NL, tokenize.NEWLINE, tokenize.INDENT, tokenize.DEDENT, tokenize.ENDMARKER)
    code = set()
    for t in tokenize.generate_tokens(io.StringIO(src).readline):
        if t.type not in skip:
            code.update(range(t.start[0], t.end[0] + 1))
    return len(code - doc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rev', default=None, help='a git revision (default: the working tree)')
    ap.add_argument('files', nargs='+')
    args = ap.parse_args()
    total = 0
    for f in args.files:
        if args.rev is None:
            src = open(f).read() if os.path.exists(f) else ''
        else:
            r = subprocess.run(['git', 'show', f'{args.rev}:{f}'], capture_output=True, text=True)
            src = r.stdout if r.returncode == 0 else ''
        n = code_lines(src)
        total += n
        print(f'{n:6d} {f}')
    print(f'{total:6d} sum')


if __name__ == '__main__':
    main()
