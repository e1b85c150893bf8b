"""The plan of a map binding (csrc/bcp_field_plan.h: the footprint geometry behind the distance-field classification, and
every shape and size bcp_set_costmaps derives from a binding) as a stand-alone host program under AddressSanitizer and
UBSan: tests/c_abi/field_plan_main.cpp includes that header alone -- it has no HIP in it -- and checks the geometric
claims (outer discs cover the footprint, inner discs lie inside it), the sizes, a table of full plans recorded before
the plan was split off, and the refusal of an oversized footprint, without a GPU."""
import host_program


def test_field_plan_under_host_sanitizers(tmp_path_factory):
    exe = host_program.build(tmp_path_factory, "field_plan_main.cpp", opt=())
    host_program.run(exe, (), "field plan ok", timeout=60)
