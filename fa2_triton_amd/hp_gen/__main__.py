from . import write_headers

print(write_headers())
