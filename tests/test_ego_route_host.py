"""The route decision of the egocentric observation (csrc/bcp_ego_route.h: which kernel a call's shape and the cell-list
facts lead to, the launch shape that goes with it, the sparse route's limit) as a stand-alone host program under
AddressSanitizer and UBSan: tests/c_abi/ego_route_main.cpp includes that header alone -- it has no HIP in it -- and checks
the table of routes, so a router that sent every call to one kernel fails here, without a GPU."""
import host_program


def test_ego_route_table_under_host_sanitizers(tmp_path_factory):
    exe = host_program.build(tmp_path_factory, "ego_route_main.cpp", opt=())
    host_program.run(exe, (), "ego route ok", timeout=60)
